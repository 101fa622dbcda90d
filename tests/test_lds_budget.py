"""How many LDS rows the traversal stack of the narrow fused frame kernels has must not show in any result: a stream of
pipelined frames — walk, connect and reconstruct parts in one launch (csrc/fs_frame.hip), at one and at two frames per launch,
without and with a source actor (the EXT flavour) — gives the same energies, published IRs and work counters with the default
rows, with rows for the tree's worst case (FS_STACK_ROWS_CAP=64: no deep store) and with 12 rows (spilling all the time).
(A 32 KiB LDS budget per workgroup, which would have derived the rows from what the other parts leave, was built and measured
negative: DESIGN.md section 10.  The test it came with stays: it is the only one that streams the EXT flavour against the caps.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DET = 8   # FS_FLAG_DETERMINISTIC
RAYS = 262144   # 131 072 pairs: 1 024 walk workgroups, the smallest frame that takes the narrow flavour (fs_frame.hip: kFrameNarrowFromBlocks)


def _stream(pkg, sc, ext):
    """one context: a stream of pipelined frames at one and at two frames per launch -> everything a reader can see"""
    ctx = pkg.Context(num_bands=sc.num_bands)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption, object_ids=sc.object_ids if ext else None)
    ctx.set_listener(sc.listener)
    src = ctx.create_source(sc.source)
    if ext:
        ctx.set_source_object(src, int(np.asarray(sc.object_ids).reshape(-1)[0]))   # the walks ignore an actor: the EXT flavour
    need = ctx.stats()["bvh_stack_need"]
    ctx.set_pipelining(2)
    out = []
    for fpl in (1, 2):
        ctx.set_frames_per_launch(fpl)
        ctx.reset_stats()
        for i in range(5):
            p = pkg.default_params(num_rays=RAYS, depth=8, seed=7100 + 10 * fpl + i, flags=DET)
            ctx.compute_energy_response_async(src, p)
            ctx.reconstruct_impulse_response_async(src, p)
        ctx.synchronize()
        st = ctx.stats()
        out += [ctx.energy_buffer(src).copy(), ctx.impulse_response(src, 0).copy(),
                np.array([st["segments"], st["connections_tested"], st["deposits"]], np.uint64)]
    assert ctx.pipeline_counters()["fused_launches"] > 0
    ctx.close()
    return need, out


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "source_actor"])
def test_stack_rows_do_not_show_in_a_stream_of_frames(pkg, scene_factory, monkeypatch, ext):
    sc = scene_factory("old_mine", 8)
    got = {}
    for cap in (None, "64", "12"):
        if cap is None:
            monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
        else:
            monkeypatch.setenv("FS_STACK_ROWS_CAP", cap)
        need, got[cap] = _stream(pkg, sc, ext)
        assert need + 1 > 22, "the scene must need more rows than the default 21 + 1 for the default rows to spill"
    e, ir, counters = got[None][0], got[None][1], got[None][2]
    assert e.any() and ir.any() and counters.all()
    for cap in ("64", "12"):
        for k, (a, b) in enumerate(zip(got[None], got[cap])):
            assert np.array_equal(a, b), (cap, k)
