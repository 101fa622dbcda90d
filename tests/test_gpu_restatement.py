"""The frame kernels against something that is NOT the oracle: the float64 model of tests/restate_walk.py (walk, connection,
evaluation and deposit written from the reference's lines, rectangles intersected analytically) gives a frame's energy
histogram and work counters, and fs_compute_energy_response must reproduce them.

For a frame of P pairs the model yields H [bands][bins] summed over the pairs it does not flag as fragile, the flagged set
Fr, the deposits D among the others and the steps S of all walks (exact: the roulette is integer arithmetic).  With G the
library's histogram and R = G - H:

  segments == planned_segments == S, connections_tested == P, |deposits - D| <= |Fr|;
  an entry is BAD when |R| > ENERGY_RTOL H + 1e-30 (ENERGY_RTOL: what tests/test_independent_restatement.py measured between
  model and oracle, times 4); at most |Fr| bins hold a bad entry, and a bad entry has 0 < R <= |Fr| energy_gain energy_clamp / P
  — a flagged pair can only ADD one deposit somewhere.

|Fr| <= 2 % of P is a condition on the inputs, asserted before the library is called.  The model's frames are computed once per
(depth, roulette, map, seed, pairs) and shared by all variants.  Shapes: 1024 pairs (waves of one subpath with the cooperative
traversal) at depth 1, 2, 4 with and without roulette, and 8192 pairs at depth 4, the smallest frame at which the library's policy
(auto_rays_per_wave, fs_capi_context.cpp: 2048 waves) leaves the cooperative kernels for walk_kernel_sparse — by policy a capped
frame gets dense waves from 131 072 pairs on only, far more than the model can serve in seconds, so the dense walk, alone and as
a part of the fused frame launch, is reached with FS_WALK_RAYS_PER_WAVE=64 (README.md) on the 1024-pair frame.  Every frame runs
on the walls cut 1 x 1 and 8 x 8: same expectation, another tree.

Measured on an MI355X: the 1024-pair frames have 0 or 1 flagged pair and no bad bin but the flagged pair's; their largest
relative difference in a good entry is 3e-7 ... 9e-7 (1.2e-6 in deterministic mode); the 8192-pair frame has 7 flagged pairs
(0.09 %), 7 more deposits than the model's unflagged ones, 5 bad bins, and 3.3e-5 as its largest difference (ENERGY_RTOL = 4e-5:
the oracle differs from the model by the same 3.3e-5 there.  It is no evaluation error but the float32 walk's drift: after a
grazing bounce one path's last node lies 0.056 cm from the model's, which changes 1 / d^2 of its 29.6 m segment by 3.8e-5).

The build-owned modes (FS_FLAG_ALL_CONNECTIONS, FS_FLAG_MIS_BALANCE, FS_FLAG_MATERIAL_LOBES) are frames of MANY contributions
per pair: Fr is then the set of flagged contributions (i, j), C = the sum over the pairs of (kf + 1)(km + 1) replaces P in
connections_tested == C, D counts the unflagged contributions that deposit, and the tolerance is the mode's (MODES in
tests/test_independent_restatement.py: 4 x what oracle and model differ by on the CPU).  A flagged contribution can still only add
one deposit of at most energy_gain energy_clamp / P, its weight being at most 1.
Measured on an MI355X, 1024 pairs: uniform and balance-heuristic weights at depth 4: 3 flagged of 16 919, 7 866 deposits against
the model's 7 863 unflagged, no bad bin; at depth 8: 24 flagged of 37 339, 21 664 against 21 643, one bad bin; lobes at depth 4 / 8:
1 / 3 flagged pairs, deposits equal, no bad bin, largest difference of a good entry 6e-7 / 6e-6; lobes with all prefixes: 30
flagged, 4 more deposits, one bad bin.  In the all-prefix frames the largest difference of an entry that is not bad is 6e-5 ...
1.9e-4: the deposit of a flagged contribution that stays below the tolerance of an occupied bin (the oracle's frame differs
from H by the same 1.92e-4 in the same bin); deposits and counters equal the oracle's in every frame.
"""
import numpy as np
import pytest

import restate_walk as rw
from test_independent_restatement import (ENERGY_RTOL, LOBE_SIGMA, LOBE_TAU, LOBES, MODES, flagged_contributions, mode_frame, mode_rtol,
                                          model_frame)

pytestmark = pytest.mark.gpu

DET, COSINE, DPOS = 8, 4, 256      # FS_FLAG_DETERMINISTIC, FS_FLAG_COSINE_SAMPLING, FS_FLAG_DOUBLE_POSITIONS
SEED = 101
GAIN = 10.0                        # energy_gain of the model's frames (the reference's); energy_clamp = 1

_ctx = {}


def context(pkg, cut, fast=False, bands=4, pipelining=0, tag="", lobes=False):
    """a context with the test scene's rectangles cut into cut x cut cells, kept for the other tests of the module; lobes: with
    the Transmission / Scattering arrays of tests/test_independent_restatement.py"""
    key = (cut, fast, bands, pipelining, tag, lobes)
    if key not in _ctx:
        sc = rw.make_test_scene()
        tri, mat = sc.triangles(cut)
        ctx = pkg.Context(num_bands=bands)
        arrays = [np.asarray(a, np.float32)[:, :bands] for a in (LOBE_TAU, LOBE_SIGMA)] if lobes else [None, None]
        ctx.set_scene(np.asarray(tri, np.float32), np.asarray(mat, np.uint16), np.asarray(sc.absorption, np.float32)[:, :bands],
                      transmission=arrays[0], scattering=arrays[1], fast=fast)
        ctx.set_listener(rw.LISTENER)
        if pipelining:
            ctx.set_pipelining(pipelining)
        _ctx[key] = (ctx, ctx.create_source(rw.SOURCE))
    return _ctx[key]


def expected(depth, roulette=True, cosine=False, pairs=1024):
    fr = model_frame(depth, roulette, cosine, SEED, num_pairs=pairs, gain=GAIN)
    assert len(fr.flagged) <= 0.02 * pairs          # a condition on the inputs (the seed), checked before the GPU is used
    assert fr.deposits > pairs // 10
    return fr


def check_frame(pkg, ctx, src, fr, pairs, depth, roulette=True, flags=0, gain=GAIN, bands=4, rtol=ENERGY_RTOL, two_sided=False, peak=1.0):
    """fr: a frame of the model, of one contribution per pair (rw.Frame: C = pairs) or of many (rw.PrefixFrame: C = the sum of
    (kf + 1)(km + 1)); nfr = its flagged contributions, each of which can only ADD one deposit of at most gain clamp / pairs (a
    weight is at most 1) somewhere"""
    p = pkg.default_params(num_rays=2 * pairs, depth=depth, seed=SEED, russian_roulette=int(roulette), flags=flags, energy_gain=gain)
    ctx.reset_stats()
    G = ctx.compute_energy_response(src, p).astype(np.float64)
    st = ctx.stats()
    assert st["segments"] == st["planned_segments"] == fr.steps
    assert st["connections_tested"] == fr.connections
    check_histogram(G, st["deposits"], fr, pairs, flags=flags, gain=gain, bands=bands, rtol=rtol, two_sided=two_sided, peak=peak,
                    what=f"pairs {pairs} depth {depth} roulette {roulette} flags {flags}")


def check_histogram(G, deposits, fr, pairs, flags=0, gain=GAIN, bands=4, rtol=ENERGY_RTOL, two_sided=False, peak=1.0, what=""):
    """check_frame's rule for a histogram G and a deposit count that the caller got from the library (one source of a batched frame:
    deposits None, the counters are the batch's).  two_sided: the frame has an order window, where a flagged contribution whose
    hit count the library and the model disagree on can also take a deposit away: the cap applies to |R| (tests/test_order_window.py).
    peak: the largest gain of the source's directivity table where it exceeds 1 (the table's factor comes after the clamp)"""
    nfr = flagged_contributions(fr)
    if deposits is not None:
        assert abs(deposits - fr.deposits) <= nfr, (deposits, fr.deposits, nfr)
    H = np.asarray(fr.H, np.float64)[:bands] * (gain / GAIN)           # (the gain is the last factor of a deposit: H is linear in it)
    allow = rtol * H + 1e-30
    if flags & DET:   # every deposit is rounded to the nearest multiple of 2^-40 (include/frequensee.h): half a quantum each
        allow = allow + np.asarray(fr.count, np.float64)[None, :] * 2.0 ** -41
    R = G - H
    bad = np.abs(R) > allow
    ok = ~bad & (H > 0.0)
    worst = float((np.abs(R)[ok] / H[ok]).max()) if ok.any() else 0.0
    print(f"{what}: flagged {nfr} deposits {deposits} / {fr.deposits} "
          f"bad bins {int(bad.any(axis=0).sum())} worst relative difference {worst:.3e}")
    assert bad.any(axis=0).sum() <= nfr, np.flatnonzero(bad.any(axis=0))
    cap = nfr * gain * 1.0 / pairs * (1.0 + 1e-5) * peak
    if two_sided:
        assert (np.abs(R[bad]) <= cap).all(), (R[bad], cap)
    else:
        assert ((R[bad] > 0.0) & (R[bad] <= cap)).all(), (R[bad], cap)
    assert G.sum() > 0.0


@pytest.mark.parametrize("roulette", [True, False], ids=["rr", "norr"])
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_small_frames(pkg, depth, roulette):
    """1024 pairs (2048 subpaths: one per wave, the cooperative traversal), walls cut 1 x 1 (22 triangles) and 8 x 8 (1408)"""
    fr = expected(depth, roulette)
    for cut in (1, 8):
        ctx, src = context(pkg, cut)
        check_frame(pkg, ctx, src, fr, 1024, depth, roulette)


@pytest.mark.parametrize("cut", [1, 8])
def test_larger_frame_on_sparse_waves(pkg, cut):
    """8192 pairs at depth 4: 16 384 subpaths, 8 per wave — walk_kernel_sparse, the connect pass on waves of 2 pairs — and the
    same frame held and flushed with pipelining on: the walk and connect parts of the fused frame launch"""
    fr = expected(4, pairs=8192)
    for pipelining in (0, 1):
        ctx, src = context(pkg, cut, pipelining=pipelining)
        check_frame(pkg, ctx, src, fr, 8192, 4)


@pytest.mark.parametrize("variant", ["deterministic", "double_positions", "device_tree", "one_band", "cosine", "pipelined_1", "pipelined_2"])
def test_variants_of_the_small_frame(pkg, variant):
    """1024 pairs at depth 4 against the SAME expectation (cosine sampling: its own): deterministic deposits (gain 1e6: the quanta
    of 2^-40 far below the energies), double positions, a tree built on the device, one band (band 0 of the four), and the frame
    held by fs_set_pipelining and flushed through the fused launch"""
    fr = expected(4, cosine=variant == "cosine")
    for cut in (1, 8):
        kw = {}
        if variant == "device_tree":
            kw["fast"] = True
        if variant == "one_band":
            kw["bands"] = 1
        if variant.startswith("pipelined"):
            kw["pipelining"] = int(variant[-1])
        ctx, src = context(pkg, cut, **kw)
        flags = {"deterministic": DET, "double_positions": DPOS, "cosine": COSINE}.get(variant, 0)
        check_frame(pkg, ctx, src, fr, 1024, 4, flags=flags, gain=1e6 if variant == "deterministic" else GAIN, bands=kw.get("bands", 4))


@pytest.mark.parametrize("pipelining", [0, 1], ids=["walk_kernel", "fused_launch"])
def test_dense_waves(pkg, monkeypatch, pipelining):
    """the dense walk (one subpath per lane), which the policy gives frames of 131 072 pairs and more, on the 1024-pair frames:
    FS_WALK_RAYS_PER_WAVE=64 is read when the context is created"""
    monkeypatch.setenv("FS_WALK_RAYS_PER_WAVE", "64")
    for depth, roulette in ((4, True), (2, False)):
        fr = expected(depth, roulette)
        for cut in (1, 8):
            ctx, src = context(pkg, cut, pipelining=pipelining, tag="dense")
            check_frame(pkg, ctx, src, fr, 1024, depth, roulette)


# ---- the build-owned modes: all prefixes (connect_all_kernel), balance-heuristic weights, lobes in the walk ---------------------------------
def mode_expected(mode, depth, bands=4):
    fr = mode_frame(mode, depth, True, SEED, 1024, gain=GAIN, bands=bands)
    assert flagged_contributions(fr) <= 0.02 * fr.connections      # a condition on the inputs, checked before the GPU is used
    assert fr.deposits > 1024 // 10
    return fr


def check_mode_frame(pkg, ctx, src, fr, mode, depth, flags=0, **kw):
    check_frame(pkg, ctx, src, fr, 1024, depth, flags=MODES[mode][0] | flags, rtol=mode_rtol(mode), **kw)


@pytest.mark.parametrize("mode,depth", [("uniform", 4), ("uniform", 8), ("balance", 4), ("balance", 8), ("lobes", 4), ("lobes", 8), ("lobes_all", 4)])
def test_mode_frames(pkg, mode, depth):
    """1024 pairs in the modes whose only definition is DESIGN.md section 8, against the model's restatement of it.  Uniform weights
    at depth 4: 25 prefix combinations per pair at most, one round of connect_all_kernel's wave; at depth 8 up to 81, a second,
    partly filled round (the model counts the pairs beyond 64 and the CPU test asserts there are some)"""
    fr = mode_expected(mode, depth)
    if depth == 8 and mode != "lobes":
        assert fr.pairs_over_64 > 0
    for cut in (1, 8):
        ctx, src = context(pkg, cut, lobes=bool(MODES[mode][0] & LOBES))
        check_mode_frame(pkg, ctx, src, fr, mode, depth)


@pytest.mark.parametrize("variant", ["deterministic", "device_tree", "one_band"])
@pytest.mark.parametrize("mode,depth", [("uniform", 8), ("lobes", 4)])
def test_variants_of_the_mode_frames(pkg, mode, depth, variant):
    """deterministic deposits (gain 1e6), a tree built on the device, one band.  With one band the uniform frame is band 0 of the
    four; the lobe frame is a frame of its own, since the lobe probabilities are band means"""
    lobes = bool(MODES[mode][0] & LOBES)
    bands = 1 if variant == "one_band" else 4
    fr = mode_expected(mode, depth, bands=bands if lobes else 4)
    for cut in (1, 8):
        ctx, src = context(pkg, cut, fast=variant == "device_tree", bands=bands, lobes=lobes)
        check_mode_frame(pkg, ctx, src, fr, mode, depth, flags=DET if variant == "deterministic" else 0,
                         gain=1e6 if variant == "deterministic" else GAIN, bands=bands)


@pytest.mark.parametrize("pipelining", [0, 1], ids=["walk_kernel", "fused_launch"])
def test_dense_waves_in_the_modes(pkg, monkeypatch, pipelining):
    """the dense walk's stores of positions, normals and lobe bits: FS_WALK_RAYS_PER_WAVE=64 as in test_dense_waves"""
    monkeypatch.setenv("FS_WALK_RAYS_PER_WAVE", "64")
    for mode, depth in (("uniform", 8), ("lobes", 4)):
        fr = mode_expected(mode, depth)
        for cut in (1, 8):
            ctx, src = context(pkg, cut, pipelining=pipelining, tag="dense", lobes=bool(MODES[mode][0] & LOBES))
            check_mode_frame(pkg, ctx, src, fr, mode, depth)
