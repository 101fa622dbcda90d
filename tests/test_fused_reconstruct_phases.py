"""The reconstruct part of the narrow fused frame kernels runs in two phases when a launch carries several frames
(csrc/fs_dev_recon.hpp: reconstruct_body_staged, reconstruct_spectral_row; one frame per launch: the one-phase body and the same
spectral row): the per-band IR set and the host ring slot it writes must equal, bit for bit, what the stand-alone
reconstruct_batch_kernel path (a context without pipelining) makes of the same energy buffer — at an IR length whose last block is partial with a tail that is no multiple of 4 samples, at a
non-default bin size, with and without FS_FLAG_SPECTRAL_IR, and for a frame whose IR is shorter than the one its ring slot
held, so that the zero-block rule has blocks to clear."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DET = 8          # FS_FLAG_DETERMINISTIC
SPECTRAL = 512   # FS_FLAG_SPECTRAL_IR
RAYS = 262144    # 1 024 walk workgroups: the narrow flavour (a smaller launch takes the wide one, whose plain rows are always one-phase)
FILLERS = 5      # frames of another source behind the ones under test: two whole groups at two frames per launch and one frame over
SHAPE = dict(sample_rate=22051, simulated_duration=1.0, bin_duration=0.0005)   # 22 051 samples = 5 blocks of 4 096 + 1 571 (= 4 * 392 + 3); 12 samples per bin
# The histogram's bins are 1 ms of delay whatever the IR's bin size: the room's paths (up to ~170 ms) fill the first 2 040 samples
# at 12 samples per bin.  far: sound 12 times slower — the same energies 12 times later, all over the IR and beyond its end.
NEAR = dict()
RING = 8         # slots of a source's ring of published IRs


def _contexts(pkg, sc):
    piped = pkg.Context(num_bands=sc.num_bands, **SHAPE)
    alone = pkg.Context(num_bands=sc.num_bands, **SHAPE)
    for c in (piped, alone):
        c.set_scene(sc.triangles, sc.material_ids, sc.absorption)
        c.set_listener(sc.listener)
    piped.set_pipelining(2)
    return piped, alone


@pytest.mark.parametrize("per_launch", [1, 2])
@pytest.mark.parametrize("flags", [0, SPECTRAL], ids=["plain", "spectral"])
def test_fused_reconstruct_equals_the_stand_alone_kernel(pkg, scene_factory, flags, per_launch):
    sc = scene_factory("starter_room", 4)
    piped, alone = _contexts(pkg, sc)
    piped.set_frames_per_launch(per_launch)
    ns = piped.num_samples
    assert ns % 4096 != 0 and (ns % 4096) % 4 != 0 and ns == alone.num_samples
    s, filler = piped.create_source(sc.source), piped.create_source(np.asarray(sc.source, np.float32) + np.float32(20.0))
    r = alone.create_source(sc.source)
    FAR = dict(sound_speed=pkg.default_params().sound_speed / 12.0)
    # The frames of source s: RING far ones — the last of them lands in the first one's ring slot —, then a near one into a slot
    # that held a far IR.  The reconstruct of a frame rides in a later launch: frames of another source follow, so that every
    # reconstruct under test is a part of a launch with full-size walks and a connect part (the drain's last launches are small:
    # the wide flavour).
    kinds = [FAR] * RING + [NEAR]
    checked = 0
    for upto in (RING, RING + 1):   # the stream up to the last far frame, then up to the near one
        if upto == RING + 1:
            kinds_now = kinds[RING:]
        else:
            kinds_now = kinds[:RING]
        for i, kw in enumerate(kinds_now):
            p = pkg.default_params(num_rays=RAYS, depth=8, seed=500 + checked + i, flags=DET | flags, **kw)
            piped.compute_energy_response_async(s, p)
            piped.reconstruct_impulse_response_async(s, p)
        for i in range(FILLERS):
            q = pkg.default_params(num_rays=RAYS, depth=8, seed=900 + i, flags=DET)
            piped.compute_energy_response_async(filler, q)
            piped.reconstruct_impulse_response_async(filler, q)
        piped.synchronize()
        e = piped.energy_buffer(s).copy()
        assert e.any()
        # the same publishes of the same energy by the kernel that only reconstructs (its ring slots go through the same history)
        # (without the deterministic flag: the installed float histogram is the frame, there is no integer one to convert)
        for _ in kinds_now:
            alone.update_energy_buffer(r, e)
            alone.reconstruct_impulse_response(r, pkg.default_params(flags=flags))
        got, want = piped.impulse_response(s, 0), alone.impulse_response(r, 0)
        assert want.any()
        if upto == RING:
            assert want[4096:].any(), "the far frames must reach late blocks"
        else:
            assert want[:4096].any() and not want[4096:].any(), "the near frame must leave the late blocks zero"
        assert np.array_equal(got, want), (upto, int(np.flatnonzero(got != want)[0]))
        for b in range(sc.num_bands):
            gb, wb = piped.band_impulse_response(s, b), alone.band_impulse_response(r, b)
            assert np.array_equal(gb, wb), (upto, b, int(np.flatnonzero(gb != wb)[0]))
        checked += len(kinds_now)
    assert piped.pipeline_counters()["publishes_by_word"] > 0   # the launches' own reconstruct parts published
    piped.close(); alone.close()
