"""The frame kernels against the float64 model of tests/restate_walk.py where a frame depends on MORE than the scene, the two end
points and the mode: a source with a directivity table and an orientation (connect_dir_kernel, connect_all_dir_kernel), with an order
window on top, walks that ignore the actor they start from (the EXT flavours of the walk and of the fused launch), and batched
frames in which every source reads its own row of the batch table.  No test here compares a kernel with the oracle or with a float32
restatement of the kernel: the model's part for all of this is rw.apply_source and the `ignore` argument of rw.walk, written from
include/frequensee.h, and tests/test_restatement_sources.py compared it with the oracle's side on the CPU first.

The acceptance rule is check_frame's of tests/test_gpu_restatement.py, unchanged: counters exact, |deposits - D| <= |Fr|, at most
|Fr| bins with a bad entry, a bad entry within |Fr| gain clamp / P (x the table's largest gain where that exceeds 1: D is the last
factor, after the clamp; with a window the cap applies to |R|).  Fr holds the contributions the model leaves out: the flagged ones
and, with a table, those whose D is too steep for the emission direction's error (rw.apply_source).  Conditions on the inputs,
asserted before the GPU is used: |Fr| <= 2 % of the contributions and more than pairs // 10 deposits — in a windowed frame the
latter holds for the frame without the window, and the window keeps at least one deposit (no placement gives 1 024 pairs a hundred
paths of order 0: such a path needs both walks to end or miss at once).

Tolerances: ENERGY_RTOL end to end and mode_rtol(mode) otherwise, as they stand — on the CPU the directional frames of depth 4 and
the all-prefix ones of depth 8 stayed within a quarter of them (tests/test_restatement_sources.py), and the ignored-actor frames
likewise.

Frames: seed 101, roulette on, 4 bands, walls cut 1 x 1 and 8 x 8; the shapes are those of tests/test_gpu_restatement.py, the
smallest at which each path is reached.  The box scene: the test scene with a closed box of material 1, actor 7, round the source;
the source's walks ignore 7, the listener's ignore the slab (actor 2).

Measured on an MI355X (the two cuts agree in every figure but the last digit of the difference); flagged (of which for D alone), the
library's deposits / the model's unflagged ones, bins with a bad entry, largest relative difference of a good entry:

  directional, cardioid   end to end 1 024: 19 (19), 653 / 634, 7, 6.7e-7;  8 192: 117 (110), 5 168 / 5 051, 15, 2.6e-5
                          uniform depth 4: 26 (23) of 16 919, 7 866 / 7 840, 5, 2.4e-4;  depth 8: 317 (293) of 37 339, 21 664 / 21 350, 15, 2.7e-4
                          balance: 8 (5), 7 866 / 7 858, 0, 3.3e-4;  lobes: 1 (0), 607 / 607, 0, 6.3e-7;  lobes_all: 134 (104), 7 536 / 7 428, 11, 1.1e-4
  variants, end to end    deterministic 7.7e-6, double positions 4.9e-7, device tree, 1 and 3 bands, dense waves 4.6e-7 ... 6.5e-7, all with the
                          19 flagged, 653 / 634 and 7 bins above;  two samples: 2, 653 / 651, 2, 4.5e-7;  cone: 6, 653 / 647, 5, 1.3e-6
  variants, uniform d 8   all 317, 21 664 / 21 350, 15, 2.7e-4 (deterministic: entries below the quantum of 2^-40 differ by all of themselves,
                          within count x 2^-41);  two samples: 66, 21 664 / 21 601, 8, 2.5e-4;  cone: 140, 21 664 / 21 527, 14, 6.9e-5
  window x table          end to end [0, 0]: 2, 10 / 10, 0, 4.3e-7;  [1, 3]: 3, 66 / 65, 1, 4.3e-7;  [2, inf): 17, 863 / 847, 8, 2.4e-6
                          uniform [0, 0]: 6, 1 047 / 1 047, 0, 2.4e-6;  [1, 3]: 24, 7 024 / 7 005, 3, 2.8e-4;  [2, inf): 77, 12 764 / 12 689, 8, 3.0e-4
  ignored actors          end to end 1 024: 0, 646 / 646, 0, 1.1e-6 (so every variant);  8 192: 5, 5 213 / 5 208, 2, 2.7e-5
                          uniform: 6 of 16 919, 7 451 / 7 448, 1, 2.5e-4 (so every variant);  lobes: 0, 610 / 610, 0, 1.3e-6
  batched                 end to end: 19 / 0 / 9 flagged, 7 / 0 / 7 bins, 5.5e-7 / 3.5e-7 / 4.3e-6;  uniform: 26 / 8 / 47, 5 / 3 / 8,
                          2.4e-4 / 5.9e-7 / 2.7e-4; the counters equal the sums

The differences of 2e-4 ... 3e-4 in the all-prefix frames are, as in tests/test_gpu_restatement.py, deposits of flagged contributions
that stay below the tolerance of an occupied bin.  No frame failed its rule: nothing in csrc changed.
"""
import numpy as np
import pytest

import restate_walk as rw
from test_gpu_restatement import DET, DPOS, GAIN, SEED, check_frame, check_histogram, context
from test_independent_restatement import LOBE_SIGMA, LOBE_TAU, LOBES, MODES
from test_order_window_cpu import LISTENER2, frame_of
from test_restatement_sources import (BOX_ACTOR, SLAB_ACTOR, SOURCES, TABLES, applied, box_scene, rtol_of, source_frame)
from test_directivity import OBLIQUE

pytestmark = pytest.mark.gpu

PAIRS = 1024
CUTS = (1, 8)


def flags_of(mode):
    return MODES[mode][0] if mode else 0


def expected(fr, mode, table="cardioid", orientation=OBLIQUE, lo=0, hi=None, depth=4, pairs=PAIRS):
    """the model's frame under the descriptor, with the conditions on the inputs"""
    a, rtol = applied(fr, mode, table, orientation, lo, hi, depth)
    whole = a if (lo, hi) == (0, None) else applied(fr, mode, table, orientation, depth=depth)[0]
    assert a.flagged <= 0.02 * a.connections, (a.flagged, a.connections)
    assert whole.deposits > pairs // 10 and a.deposits > 0
    return a, rtol


def describe(ctx, s, table, orientation, lo, hi, bands=4):
    if table is not None:
        ctx.set_source_orientation(s, orientation)
        ctx.set_source_directivity(s, TABLES[table][:bands])
    if (lo, hi) != (0, None):
        ctx.set_source_order_window(s, lo, hi)


def check_described(pkg, ctx, a, rtol, mode, depth, table="cardioid", orientation=OBLIQUE, lo=0, hi=None, pairs=PAIRS, flags=0, gain=GAIN,
                    bands=4, position=rw.SOURCE):
    """one frame of a new source with the descriptor against the model's a"""
    s = ctx.create_source(position)
    try:
        describe(ctx, s, table, orientation, lo, hi, bands)
        peak = max(1.0, float(TABLES[table].max())) if table is not None else 1.0
        check_frame(pkg, ctx, s, a, pairs, depth, flags=flags_of(mode) | flags, gain=gain, bands=bands, rtol=rtol,
                    two_sided=(lo, hi) != (0, None), peak=peak)
    finally:
        ctx.destroy_source(s)


# ---- directional frames ----------------------------------------------------------------------------------------------------------------------
DIRECTIONAL = [(None, 4, 1024), (None, 4, 8192), ("uniform", 4, 1024), ("uniform", 8, 1024), ("balance", 4, 1024), ("lobes", 4, 1024),
               ("lobes_all", 4, 1024)]


@pytest.mark.parametrize("mode,depth,pairs", DIRECTIONAL, ids=[f"{m or 'end_to_end'}_d{d}_{p}" for m, d, p in DIRECTIONAL])
def test_directional_frames(pkg, mode, depth, pairs):
    """cardioid(4), facing OBLIQUE.  End to end: 1 024 pairs, one subpath per wave (connect_dir_kernel), and 8 192, the sparse-wave
    evaluation where lane i holds segment i.  All prefixes (connect_all_dir_kernel): depth 4, one round of the wave's 64 combinations, and
    depth 8 with a second, partly filled round; balance-heuristic weights; lobes in the walk, end to end and with all prefixes"""
    fr = source_frame(mode, depth, SEED, pairs)
    if mode == "uniform" and depth == 8:
        assert fr.pairs_over_64 > 0
    a, rtol = expected(fr, mode, depth=depth, pairs=pairs)
    if mode in ("uniform", "balance", "lobes_all"):
        assert a.connection_ray > pairs // 4 and a.walk_ray > pairs           # both sources of the emission direction
    for cut in CUTS:
        ctx, _ = context(pkg, cut, lobes=bool(flags_of(mode) & LOBES))
        check_described(pkg, ctx, a, rtol, mode, depth, pairs=pairs)


VARIANTS = ["deterministic", "double_positions", "device_tree", "bands_1", "bands_3", "dense_waves", "two_samples", "cone"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode,depth", [(None, 4), ("uniform", 8)], ids=["end_to_end", "uniform_d8"])
def test_variants_of_the_directional_frames(pkg, monkeypatch, mode, depth, variant):
    """the same two model frames: deterministic deposits (gain 1e6), double positions (the connection ray comes from the double end
    points), a tree built on the device, 1 and 3 bands (1 and 4 are compile-time instances of the all-prefix kernel, 3 takes its
    run-time band count; the frames are the first so many bands of the four), dense waves (FS_WALK_RAYS_PER_WAVE=64, read when the
    context is created), the K = 2 table (k = 0 always) and the cone's 181 samples.  The library refuses FS_FLAG_DOUBLE_POSITIONS with
    the all-connections modes (include/frequensee.h): that variant is the end-to-end frame's alone"""
    if mode is not None and variant == "double_positions":
        ctx, s = context(pkg, 1)
        with pytest.raises(pkg.FrequenSeeError) as ei:
            ctx.compute_energy_response(s, pkg.default_params(num_rays=2 * PAIRS, depth=depth, seed=SEED, flags=flags_of(mode) | DPOS))
        assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
        return
    fr = source_frame(mode, depth, SEED, PAIRS)
    table = {"two_samples": "two", "cone": "cone"}.get(variant, "cardioid")
    a, rtol = expected(fr, mode, table, depth=depth)
    kw = {}
    if variant == "device_tree":
        kw["fast"] = True
    if variant.startswith("bands"):
        kw["bands"] = int(variant[-1])
    if variant == "dense_waves":
        monkeypatch.setenv("FS_WALK_RAYS_PER_WAVE", "64")
        kw["tag"] = "dense"
    flags = {"deterministic": DET, "double_positions": DPOS}.get(variant, 0)
    for cut in CUTS:
        ctx, _ = context(pkg, cut, **kw)
        check_described(pkg, ctx, a, rtol, mode, depth, table, flags=flags, gain=1e6 if variant == "deterministic" else GAIN,
                        bands=kw.get("bands", 4))


@pytest.mark.parametrize("lo,hi", [(0, 0), (1, 3), (2, None)], ids=["direct", "early", "late"])
@pytest.mark.parametrize("mode", [None, "uniform"], ids=["end_to_end", "uniform"])
def test_window_and_table_against_the_model(pkg, mode, lo, hi):
    """window x table, each against the model directly; the listener in view of the source (LISTENER2 of tests/test_order_window_cpu.py:
    behind the slab no path has order 0).  From there the source is seen at 150 degrees from OBLIQUE, on the cardioid's floor: end to
    end the contributions left out for D alone make 30 flagged of 1 024 in [2, inf), past the 2 % a frame may have, so the end-to-end
    frames take the cardioid on a floor of 0.1 (17 of 1 024; TABLES of tests/test_restatement_sources.py); the cap stays"""
    fr = frame_of(mode, LISTENER2)
    table = "cardioid_raised" if mode is None else "cardioid"
    a, rtol = expected(fr, mode, table, lo=lo, hi=hi)
    for cut in CUTS:
        ctx, _ = context(pkg, cut, tag="sources_in_view")
        ctx.set_listener(LISTENER2)
        check_described(pkg, ctx, a, rtol, mode, 4, table, lo=lo, hi=hi)


# ---- ignored actors ------------------------------------------------------------------------------------------------------------------------------
_box = {}


def box_context(pkg, cut, fast=False, pipelining=0, tag="", lobes=False):
    key = (cut, fast, pipelining, tag, lobes)
    if key not in _box:
        sc = box_scene()
        tri, mat = sc.triangles(cut)
        ctx = pkg.Context(num_bands=4)
        arrays = [np.asarray(a, np.float32) for a in (LOBE_TAU, LOBE_SIGMA)] if lobes else [None, None]
        ctx.set_scene(np.asarray(tri, np.float32), np.asarray(mat, np.uint16), np.asarray(sc.absorption, np.float32),
                      transmission=arrays[0], scattering=arrays[1], object_ids=np.asarray(sc.object_ids(cut), np.uint32), fast=fast)
        ctx.set_listener(rw.LISTENER)
        ctx.set_listener_object(SLAB_ACTOR)
        if pipelining:
            ctx.set_pipelining(pipelining)
        s = ctx.create_source(rw.SOURCE)
        ctx.set_source_object(s, BOX_ACTOR)
        _box[key] = (ctx, s)
    return _box[key]


def box_expected(mode, pairs=PAIRS):
    fr = source_frame(mode, 4, SEED, pairs, box=True)
    nfr = fr.flagged if isinstance(fr.flagged, int) else len(fr.flagged)
    assert nfr <= 0.02 * fr.connections and fr.deposits > pairs // 10
    return fr


IGNORED = [(None, 1024), (None, 8192), ("uniform", 1024), ("lobes", 1024)]


@pytest.mark.parametrize("mode,pairs", IGNORED, ids=[f"{m or 'end_to_end'}_{p}" for m, p in IGNORED])
def test_ignored_actors(pkg, mode, pairs):
    """the source sealed in its own box, the listener's walks passing through the slab, the connection seeing both: end to end on waves
    of one subpath and on sparse waves, all prefixes, and lobes (transmitted steps with an ignored actor)"""
    fr = box_expected(mode, pairs)
    for cut in CUTS:
        ctx, s = box_context(pkg, cut, lobes=mode == "lobes")
        check_frame(pkg, ctx, s, fr, pairs, 4, flags=flags_of(mode), rtol=rtol_of(mode))


@pytest.mark.parametrize("variant", ["device_tree", "dense_waves", "pipelined_1", "pipelined_2"])
@pytest.mark.parametrize("mode", [None, "uniform"], ids=["end_to_end", "uniform"])
def test_variants_of_the_ignored_actor_frames(pkg, monkeypatch, mode, variant):
    """a tree built on the device, dense waves, and the frame given to a context with fs_set_pipelining(1) and (2): the EXT flavours of
    the walk and of the fused launch"""
    fr = box_expected(mode)
    kw = {}
    if variant == "device_tree":
        kw["fast"] = True
    if variant == "dense_waves":
        monkeypatch.setenv("FS_WALK_RAYS_PER_WAVE", "64")
        kw["tag"] = "dense"
    if variant.startswith("pipelined"):
        kw["pipelining"] = int(variant[-1])
    for cut in CUTS:
        ctx, s = box_context(pkg, cut, **kw)
        check_frame(pkg, ctx, s, fr, PAIRS, 4, flags=flags_of(mode), rtol=rtol_of(mode))


def test_nothing_ignored_nothing_deposited(pkg):
    """the control of the CPU leg on the device: without its actor ignored the source's walks stay in the box, and the connection,
    which ignores nothing, finds every pair blocked"""
    fr = source_frame(None, 4, SEED, PAIRS, box=True, ignore=(rw.NO_OBJECT, rw.NO_OBJECT))
    assert fr.deposits == 0
    ctx, s = box_context(pkg, 8, tag="sealed")
    ctx.set_source_object(s)
    ctx.set_listener_object()
    ctx.reset_stats()
    G = ctx.compute_energy_response(s, pkg.default_params(num_rays=2 * PAIRS, depth=4, seed=SEED, russian_roulette=1, energy_gain=GAIN))
    st = ctx.stats()
    assert st["segments"] == fr.steps and st["connections_tested"] == PAIRS
    assert abs(st["deposits"] - 0) <= len(fr.flagged) and (len(fr.flagged) > 0 or not G.any())


# ---- batched sources: every source reads its own row of the batch table ---------------------------------------------------------------------------
DESCRIPTORS = [("cardioid", OBLIQUE, 0, None), (None, (1.0, 0.0, 0.0), 1, 3), ("cone", (-1.0, 0.2, 0.1), 2, None)]


@pytest.mark.parametrize("mode", [None, "uniform"], ids=["end_to_end", "uniform"])
def test_batched_sources_against_their_own_frames(pkg, mode):
    """one fs_compute_energy_response_batch_async of three sources at three places with three descriptors (a table; a window; another
    table, another orientation and another window): every source's histogram against ITS model frame, the counters against the sums"""
    exp = []
    for position, (table, orientation, lo, hi) in zip(SOURCES, DESCRIPTORS):
        fr = source_frame(mode, 4, SEED, PAIRS, source=position)
        exp.append(expected(fr, mode, table, orientation, lo, hi))
    p = pkg.default_params(num_rays=2 * PAIRS, depth=4, seed=SEED, russian_roulette=1, flags=flags_of(mode), energy_gain=GAIN)
    for cut in CUTS:
        ctx, _ = context(pkg, cut, tag="batch")
        srcs = [ctx.create_source(position) for position in SOURCES]
        try:
            for s, (table, orientation, lo, hi) in zip(srcs, DESCRIPTORS):
                describe(ctx, s, table, orientation, lo, hi)
            ctx.reset_stats()
            ctx.compute_energy_response_batch_async(srcs, p)
            ctx.synchronize()
            st = ctx.stats()
            assert st["segments"] == st["planned_segments"] == sum(a.steps for a, _ in exp)
            assert st["connections_tested"] == sum(a.connections for a, _ in exp)
            assert abs(st["deposits"] - sum(a.deposits for a, _ in exp)) <= sum(a.flagged for a, _ in exp)
            for k, (s, (a, rtol), (table, _, lo, hi)) in enumerate(zip(srcs, exp, DESCRIPTORS)):
                peak = max(1.0, float(TABLES[table].max())) if table is not None else 1.0
                check_histogram(ctx.energy_buffer(s).astype(np.float64), None, a, PAIRS, flags=flags_of(mode), rtol=rtol,
                                two_sided=(lo, hi) != (0, None), peak=peak, what=f"batched {mode} cut {cut} source {k}")
        finally:
            for s in srcs:
                ctx.destroy_source(s)
