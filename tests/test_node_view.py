"""The 48-byte node view the chip-filling flavour of the fused frame kernel walks (fs_internal.hpp: ViewRec).

1. The view is an exact restatement of the committed tree: every node record decodes to its NodeQ4's origin, steps (as
   float bits) and plane words, every used slot's reference reaches exactly that child — the node it pointed to, or its
   triangles and their normals, byte for byte — and every record is reached exactly once from the root.  After a commit of
   either kind, a refit, fs_scene_update_triangles and fs_scene_set_object_transforms.
2. Frames traced through the fused narrow launch (131 072 pairs: the smallest frame that reaches it) equal the same frames
   traced unpipelined bit for bit in deterministic mode: energies, published IRs and the work counters.
3. A scene committed without its view takes another route to the same bits; the size rule at its boundary.
4. The empty scene and a tree of one node.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_check as tc  # noqa: E402

DET = 8   # FS_FLAG_DETERMINISTIC: integer deposits, the same energy however the frame is scheduled
VIEW_WHAT = {"view": (11, np.dtype("<u4")), "view_nrm": (12, tc.FLOAT4_DT), "view_of_leaf": (13, np.dtype("<u4"))}
ABSORPTION = np.array([[0.3], [0.5], [0.8]], np.float32)
NARROW_RAYS = 262144   # 131 072 pairs, 1 024 walk workgroups: the fewest that take the narrow flavour


def fetch_view(ctx, name):
    """one of the view's arrays through fs_debug_scene_snapshot (no bytes: the scene has no view)"""
    fn = ctx.lib.fs_debug_scene_snapshot
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    what, dt = VIEW_WHAT[name]
    n = C.c_size_t(0)
    fn(ctx.h, what, None, 0, C.byref(n))
    buf = np.zeros(n.value, np.uint8)
    if n.value:
        ctx.check(fn(ctx.h, what, buf.ctypes.data, n.value, C.byref(n)))
    a = buf.view(dt)
    return a.reshape(-1, 12) if name == "view" else a


def set_node_view(ctx, on):
    fn = ctx.lib.fs_debug_set_node_view
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32]
    ctx.check(fn(ctx.h, 1 if on else 0))


def check_view(ctx):
    """the view against NodeQ4 / Tri48 / the normals as they stand; returns (leaf sizes seen, largest slot offset)"""
    nodes, tri48, nrm = tc.fetch(ctx, "nodes"), tc.fetch(ctx, "tri48"), tc.fetch(ctx, "nrm")
    U, Un, of_leaf = fetch_view(ctx, "view"), fetch_view(ctx, "view_nrm"), fetch_view(ctx, "view_of_leaf")
    n, T = nodes.shape[0], tri48.shape[0]
    assert U.shape[0] == n + T and Un.shape[0] == n + T and of_leaf.shape[0] == T
    tri_words = tri48.view("<u4").reshape(T, 12)
    nrm_words, un_words = nrm.view("<u4").reshape(T, 4), Un.view("<u4").reshape(n + T, 4)
    used = tc._used(nodes)
    visits = np.zeros(n + T, np.int64)
    leaf_sizes, max_off = set(), 0
    todo = [(0, 0)]                                  # (node index, view record): the root is record 0
    while todo:
        i, r = todo.pop()
        visits[r] += 1
        w, q = U[r], nodes[i]
        assert w[0:3].tobytes() == np.array([q["ox"], q["oy"], q["oz"]], "<f4").tobytes(), ("origin", i)
        assert [int(v) for v in w[3:9]] == [int(q[k]) for k in ("lox", "loy", "loz", "hix", "hiy", "hiz")], ("planes", i)
        G, cb8, E = int(w[9]), int(w[10]), int(w[11])
        steps = np.array([((E >> (8 * k)) & 0xFF) << 23 for k in range(3)], "<u4")
        assert steps.tobytes() == np.array([q["sx"], q["sy"], q["sz"]], "<f4").tobytes() and E >> 24 == 0, ("steps", i)
        assert cb8 % 8 == 0 and 0 < cb8 // 8 <= n + T
        off = 0
        for c in range(4):
            g = (G >> (8 * c)) & 0xFF
            if not used[i, c]:
                assert g == 0, ("empty slot", i, c)
                continue
            ref = cb8 + g
            rec, leaf, cnt = ref >> 3, (ref >> 2) & 1, (ref & 3) + 1
            assert g >> 3 == off and rec == cb8 // 8 + off and ref < 1 << 30, ("slot order", i, c)
            max_off = max(max_off, off)
            link = int(q["child"][c])
            if link >= 0:
                assert leaf == 0 and cnt == 1, ("inner", i, c)
                todo.append((link, rec))
                off += 1
            else:
                first, count = (~link) >> 2, ((~link) & 3) + 1
                assert leaf == 1 and cnt == count, ("leaf", i, c)
                leaf_sizes.add(count)
                for j in range(count):
                    visits[rec + j] += 1
                    assert U[rec + j].tobytes() == tri_words[first + j].tobytes(), ("triangle", i, c, j)
                    assert un_words[rec + j].tobytes() == nrm_words[first + j].tobytes(), ("normal", i, c, j)
                    assert of_leaf[first + j] == rec + j, ("leaf map", i, c, j)
                off += count
    assert np.all(visits == 1), "a record is reached %d times" % int(visits[visits != 1][0])
    return leaf_sizes, max_off


def _scene(pkg, name):
    """(triangles, materials, absorption, actor ids or None, fast commit, FS_BVH_LEAF or None)"""
    rng = np.random.default_rng(0x48)
    if name == "box":
        sc = pkg.scenes.shoebox(1)
        return sc.triangles, sc.material_ids, sc.absorption, (np.arange(12) // 4 + 5).astype(np.uint32), False, None
    if name == "single":
        tri = np.array([[[0, 0, 0], [300, 0, 0], [0, 300, 50]]], np.float32)
        return tri, np.zeros(1, np.uint16), ABSORPTION, np.array([9], np.uint32), False, None
    if name == "starter_room":
        sc = pkg.scenes.starter_room(4)
        T = sc.triangles.shape[0]
        return sc.triangles, sc.material_ids, sc.absorption, (np.arange(T) // 64 + 5).astype(np.uint32), False, None
    T = {"zero_area": 300, "leaf4": 3000, "device": 1500}[name]
    tri = tc.soup("zero_area" if name == "zero_area" else "uniform", T, rng).astype(np.float32)
    return tri, rng.integers(0, 3, T).astype(np.uint16), ABSORPTION, (np.arange(T) // 3 + 5).astype(np.uint32), name == "device", \
        "4" if name == "leaf4" else None


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "single", "starter_room", "zero_area", "leaf4", "device"])
def test_view_restates_the_tree(pkg, monkeypatch, name):
    tri, mat, ab, obj, fast, leaf = _scene(pkg, name)
    if leaf is None:
        monkeypatch.delenv("FS_BVH_LEAF", raising=False)
    else:
        monkeypatch.setenv("FS_BVH_LEAF", leaf)
    ctx = pkg.Context(num_bands=ab.shape[1])
    ctx.set_scene(tri, mat, ab, object_ids=obj, fast=fast)
    hdr = tc.fetch(ctx, "header")
    assert hdr["fast"] == int(fast)
    sizes, max_off = check_view(ctx)
    print(f"{name}: {hdr['nodes']} nodes, {hdr['tris']} triangles, leaf sizes {sorted(sizes)}, largest slot offset {max_off}")
    if name == "single":
        assert hdr["nodes"] == 1 and sizes == {1}
    if name == "leaf4":
        assert {3, 4} <= sizes and max_off == 12
    layout = fetch_view(ctx, "view_of_leaf").copy()
    ctx.refit()
    check_view(ctx)
    rng = np.random.default_rng(7)
    k = min(tri.shape[0], 40)
    first = tri.shape[0] - k
    ctx.update_triangles(first, tri[first:] + rng.normal(0, 20, (k, 3, 3)).astype(np.float32))
    check_view(ctx)                                  # the records are new already, the boxes still old: in both
    ctx.refit()
    check_view(ctx)
    ids = np.unique(obj)[:3]
    m = np.tile(np.eye(3, 4, dtype=np.float32), (ids.shape[0], 1, 1))
    m[:, :, 3] = rng.uniform(-30, 30, (ids.shape[0], 3))
    ctx.set_object_transforms(ids, m)
    check_view(ctx)
    ctx.refit()
    check_view(ctx)
    assert np.array_equal(fetch_view(ctx, "view_of_leaf"), layout)   # the layout follows the topology: a refit keeps it
    ctx.close()


# ---- the fused narrow launch ---------------------------------------------------------------------------------------------------
COUNTERS = ("frames", "rays", "segments", "connections_tested", "deposits")
N_FRAMES = 5


def _frames(pkg):
    return [pkg.default_params(num_rays=NARROW_RAYS, depth=8, seed=0x4800 + i, flags=DET) for i in range(N_FRAMES)]


def _make(pkg, scene, view=True, ext=False):
    tri, mat, ab, listener, source = scene
    ctx = pkg.Context(num_bands=ab.shape[1])
    if not view:
        set_node_view(ctx, False)
    obj = (np.arange(tri.shape[0]) // 64 + 5).astype(np.uint32) if ext and tri.shape[0] else None
    ctx.set_scene(tri, mat, ab, object_ids=obj)
    ctx.set_listener(listener)
    src = ctx.create_source(source)
    if ext:
        ctx.set_source_object(src, 6)               # the walks that start at the source skip that actor's triangles
    return ctx, src


def _stream(pkg, ctx, src, pipelining=None, per_launch=1):
    """N_FRAMES frames and their IRs; what is left at the end: (energy, IR, counters)"""
    if pipelining:
        ctx.set_pipelining(pipelining)
        ctx.set_frames_per_launch(per_launch)
    ctx.reset_stats()
    for p in _frames(pkg):
        ctx.compute_energy_response_async(src, p)
        ctx.reconstruct_impulse_response_async(src, p)
    ctx.synchronize()
    st = ctx.stats()
    return ctx.energy_buffer(src).copy(), ctx.impulse_response(src, 0).copy(), {k: st[k] for k in COUNTERS}


def _named_scene(pkg, scene_factory, name):
    if name == "starter_room":
        sc = scene_factory("starter_room", 4)
    else:
        sc = scene_factory("shoebox", 1)
    return sc.triangles, sc.material_ids, sc.absorption, sc.listener, sc.source


_plain = {}


def _reference(pkg, key, scene, **kw):
    """the frames traced unpipelined (the NodeQ4 path), once per configuration"""
    if key not in _plain:
        ctx, src = _make(pkg, scene, **kw)
        _plain[key] = _stream(pkg, ctx, src)
        ctx.close()
        assert _plain[key][2]["rays"] > 0 and (key == "empty" or (_plain[key][0].any() and _plain[key][2]["deposits"] > 0))
    return _plain[key]


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "energy")
    assert np.array_equal(got[1], want[1]), (what, "IR")
    assert got[2] == want[2], (what, got[2], want[2])


@pytest.mark.gpu
@pytest.mark.parametrize("per_launch", [1, 2, 4])
@pytest.mark.parametrize("name", ["starter_room", "box"])
def test_fused_narrow_frames_equal_the_unpipelined_ones(pkg, scene_factory, monkeypatch, name, per_launch):
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    scene = _named_scene(pkg, scene_factory, name)
    want = _reference(pkg, name, scene)
    ctx, src = _make(pkg, scene)
    assert fetch_view(ctx, "view").shape[0] > 0
    _same(_stream(pkg, ctx, src, pipelining=2, per_launch=per_launch), want, (name, per_launch))
    ctx.close()


@pytest.mark.gpu
def test_fused_narrow_frames_source_inside_an_actor(pkg, scene_factory, monkeypatch):
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    scene = _named_scene(pkg, scene_factory, "starter_room")
    want = _reference(pkg, "starter_room/ext", scene, ext=True)
    assert want[2] != _reference(pkg, "starter_room", scene)[2]      # ignoring the actor changes the frames
    ctx, src = _make(pkg, scene, ext=True)
    _same(_stream(pkg, ctx, src, pipelining=2, per_launch=2), want, "ext")
    ctx.close()


@pytest.mark.gpu
def test_fused_narrow_frames_with_a_spilling_stack(pkg, scene_factory, monkeypatch):
    """12 LDS rows: the deep store moves the view's references in and out as the opaque words they are"""
    scene = _named_scene(pkg, scene_factory, "starter_room")
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    want = _reference(pkg, "starter_room", scene)
    monkeypatch.setenv("FS_STACK_ROWS_CAP", "12")
    ctx, src = _make(pkg, scene)
    assert ctx.stats()["bvh_stack_need"] + 1 > 13, "the tree never needs the deep store"
    _same(_stream(pkg, ctx, src, pipelining=2, per_launch=2), want, "cap 12")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [None, "12"])
def test_scene_without_its_view_takes_another_route_to_the_same_bits(pkg, scene_factory, monkeypatch, cap):
    """cap = None: the wide flavour; cap = 12 leaves the wide flavour its worst-case rows too (the cap bounds the narrow one)"""
    scene = _named_scene(pkg, scene_factory, "starter_room")
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    want = _reference(pkg, "starter_room", scene)
    if cap:
        monkeypatch.setenv("FS_STACK_ROWS_CAP", cap)
    ctx, src = _make(pkg, scene, view=False)
    assert fetch_view(ctx, "view").shape[0] == 0 and fetch_view(ctx, "view_of_leaf").shape[0] == 0
    _same(_stream(pkg, ctx, src, pipelining=2, per_launch=2), want, "no view")
    ctx.update_triangles(0, scene[0][:8])            # the movers find no view to follow
    ctx.refit()
    assert fetch_view(ctx, "view").shape[0] == 0
    set_node_view(ctx, True)                         # the next commit builds it again
    ctx.set_scene(scene[0], scene[1], scene[2])
    check_view(ctx)
    ctx.close()


def test_size_rule_at_its_boundary(pkg):
    """records x 48 B is the request's 32-bit byte offset: 89 478 485 records fit, one more does not"""
    fits = pkg._capi.load().fs_debug_node_view_fits
    fits.restype = C.c_int
    fits.argtypes = [C.c_uint64, C.c_uint64]
    last = 0xFFFFFFFF // 48
    assert last == 89478485 and last < 1 << 27
    for nodes in (1, 1000, last // 3):
        assert fits(nodes, last - nodes) == 1
        assert fits(nodes, last - nodes + 1) == 0
    assert fits(last, 0) == 1 and fits(last + 1, 0) == 0
    assert fits(1, 0) == 1 and fits(1 << 40, 1 << 40) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty", "one_node"])
def test_empty_scene_and_one_node_tree(pkg, monkeypatch, name):
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    if name == "empty":
        tri, mat = np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.uint16)
    else:
        tri, mat = np.array([[[-400, -400, -150], [900, -400, -150], [-400, 900, -150]]], np.float32), np.zeros(1, np.uint16)
    scene = (tri, mat, ABSORPTION[:, :1], np.array([300, 0, 0], np.float32), np.array([0, 100, 50], np.float32))
    want = _reference(pkg, name, scene)
    ctx, src = _make(pkg, scene)
    if name == "empty":
        assert fetch_view(ctx, "view").shape[0] == 0
    else:
        assert tc.fetch(ctx, "header")["nodes"] == 1
        check_view(ctx)
    _same(_stream(pkg, ctx, src, pipelining=2, per_launch=2), want, name)
    ctx.close()
