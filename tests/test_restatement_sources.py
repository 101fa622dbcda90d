"""What a SOURCE'S DESCRIPTOR and the IGNORED ACTORS do to a frame, by the float64 model of tests/restate_walk.py, on the CPU: the
model's part for them (rw.apply_source: directivity table, orientation, order window; the `ignore` argument of rw.walk) is written
from the prose of include/frequensee.h and is compared here, pair by pair, with what the oracle's side gives — before
tests/test_gpu_restatement_sources.py holds the kernels to the model.

  directivity      the model's directional contributions against test_directivity.restate, the per-pair restatement assembled from
                   the oracle's exported pieces in float32: end-to-end frames and the frames of "uniform", "balance", "lobes" and
                   "lobes_all", depth 4 and 8, seeds 101 / 202 / 303, the tables cardioid(4), cone(4) and a two-sample table (K = 2:
                   k is always 0), orientation OBLIQUE
  ignored actors   the model against the oracle's compute_energy(pair_begin = i, pair_end = i + 1) with source_object /
                   listener_object on the box scene: the test scene with a closed box of material 1 round the source (actor 7;
                   room 1, slab 2); the source's walks ignore 7, the listener's ignore 2 and pass through the slab, the connection
                   ignores nothing

The frames, the tables and the box scene are built here and shared with the GPU tests.
"""
import numpy as np
import pytest

import restate_walk as rw
from test_directivity import OBLIQUE, cardioid, cone, restate
from test_independent_restatement import (ALLC, COSINE, ENERGY_RTOL, LOBE_SIGMA, LOBE_TAU, LOBES, MIS, MODES, DIRECTIONAL_RTOL, mode_frame,
                                          mode_rtol, mode_scene, model_frame, model_scene)

SEEDS = (101, 202, 303)


def two_sample(bands):
    """K = 2: one interval, k = 0 for every direction; 1.0 ahead, 0.25 ... 0.1 behind"""
    return np.stack([[1.0, 0.25 / (1.0 + 0.5 * b)] for b in range(bands)]).astype(np.float32)


TABLES = {"cardioid": cardioid(4), "cone": cone(4), "two": two_sample(4), "cardioid_raised": cardioid(4, floor=0.1)}
# The cardioid's floor of 0.02 is where D is smallest and, in the bands of a high power, steep against its size.  In two of the CPU leg's
# frames the contributions left out for D alone push the flagged ones past the 2 % a frame may have: end to end at depth 8, seed 101
# (21 of 1 024) and "lobes_all" at depth 8, seed 202 (229 of 9 510; its tolerance is the tightest of the modes).  The cap stays; these
# two frames get the cardioid on a floor of 0.1 (11 of 1 024, 153 of 9 510).
RAISED = {(None, 8), ("lobes_all", 8)}


def tables_of(mode, depth):
    return ["cardioid_raised" if (mode, depth) in RAISED else "cardioid", "cone", "two"]
BOX, BOX_ACTOR, ROOM_ACTOR, SLAB_ACTOR = ((600.0, 800.0), (500.0, 700.0), (200.0, 400.0)), 7, 1, 2
SOURCES = [rw.SOURCE, (400.0, 1500.0, 600.0), (2000.0, 300.0, 150.0)]


def rtol_of(mode, directional=False, depth=4):
    """the tolerance a frame is judged with: ENERGY_RTOL end to end, the mode's otherwise; a directional frame's own entry where
    tests/test_independent_restatement.py has one for the mode and the depth"""
    if directional and (mode, depth) in DIRECTIONAL_RTOL:
        return DIRECTIONAL_RTOL[(mode, depth)]
    return ENERGY_RTOL if mode is None else mode_rtol(mode)


# ---- the frames ------------------------------------------------------------------------------------------------------------------------------
def box_scene(lobes=False):
    """rw.make_test_scene() with actor ids (room 1, slab 2) and a closed box [600, 800] x [500, 700] x [200, 400] of material 1,
    actor 7, round rw.SOURCE"""
    sc = rw.make_test_scene()
    for k, r in enumerate(sc.rects):
        r.object = ROOM_ACTOR if k < 5 else SLAB_ACTOR
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for c in BOX[axis]:
            sc.rects.append(rw.Rect(axis, c, (BOX[u][0], BOX[v][0]), (BOX[u][1], BOX[v][1]), 1, BOX_ACTOR))
    if lobes:
        sc.set_lobes(LOBE_TAU, LOBE_SIGMA)
    return sc


_frames = {}


def source_frame(mode, depth, seed, pairs, source=rw.SOURCE, box=False, ignore=(BOX_ACTOR, SLAB_ACTOR), gain=10.0):
    """the model's frame with its pairs kept; mode None: the end-to-end connection, else one of MODES.  The test scene seen from
    rw.SOURCE: the cached frames of model_frame / mode_frame; another source, or the box scene with its ignored actors: the same
    constructor calls.  End to end beyond depth 4 the frame carries the bound per axis like the frames of the modes: the scalar
    rule passes 0.1 cm after 8 turns, and a connection ray's error (bounds / length) then flags 3 % of a frame for D alone"""
    if not box and tuple(source) == tuple(rw.SOURCE) and (mode is not None or depth <= 4):
        if mode is None:
            return model_frame(depth, True, False, seed, pairs, gain, keep_pairs=True)
        return mode_frame(mode, depth, True, seed, pairs, gain, keep_pairs=True)
    key = (mode, depth, seed, pairs, tuple(source), box, ignore if box else None, gain)
    if key not in _frames:
        flags = MODES[mode][0] if mode else 0
        sc = box_scene(bool(flags & LOBES)) if box else rw.make_test_scene()
        if flags & LOBES and not box:
            sc.set_lobes(LOBE_TAU, LOBE_SIGMA)
        prm = rw.Params(bands=4, seed=seed, depth=depth, russian_roulette=True, cosine=bool(flags & COSINE), lobes=bool(flags & LOBES),
                        energy_gain=gain, axis_bounds=mode is not None or depth > 4)
        kw = {"ignore": ignore} if box else {}
        if flags & (ALLC | MIS):
            _frames[key] = rw.PrefixFrame(sc, prm, source, rw.LISTENER, pairs, balance=bool(flags & MIS), keep_pairs=True, **kw)
        else:
            _frames[key] = rw.Frame(sc, prm, source, rw.LISTENER, pairs, keep_pairs=True, **kw)
    return _frames[key]


_applied = {}


def applied(fr, mode, table=None, orientation=OBLIQUE, lo=0, hi=None, depth=4):
    """rw.apply_source of a frame, cached by the frame's identity: (Applied, the tolerance it was made for).  table: a key of TABLES
    or an array"""
    key = (id(fr), table if isinstance(table, (str, type(None))) else id(table), tuple(orientation), lo, hi)
    if key not in _applied:
        rtol = rtol_of(mode, table is not None, depth)
        T = TABLES[table] if isinstance(table, str) else table
        _applied[key] = (rw.apply_source(fr, None if T is None else T.tolist(), orientation, lo, hi, rtol), rtol, fr)
    return _applied[key][:2]


# ---- the model's own additions by hand -----------------------------------------------------------------------------------------------------
def test_directivity_factor_by_hand():
    """theta_k = k pi / (K - 1) gives T[b][k] exactly where the knot is met, the midpoint the mean, theta = pi the last sample
    (k = K - 2, t = 1); the orientation is normalised; K = 2 is one interval"""
    import math
    T = [[1.0, 0.5, 0.25, 0.0, 2.0], [3.0, 3.0, 3.0, 3.0, 3.0]]
    at = lambda deg: (math.cos(math.radians(deg)), math.sin(math.radians(deg)), 0.0)
    for f in ((1.0, 0.0, 0.0), (7.5, 0.0, 0.0)):
        assert rw.directivity(T, f, at(0.0))[0] == [1.0, 3.0]
        assert rw.directivity(T, f, at(22.5))[0] == pytest.approx([0.75, 3.0], rel=1e-12)
        assert rw.directivity(T, f, at(45.0))[0] == pytest.approx([0.5, 3.0], rel=1e-12)
        assert rw.directivity(T, f, at(112.5))[0] == pytest.approx([0.125, 3.0], rel=1e-12)
        D, slope, k = rw.directivity(T, f, at(180.0))
        assert k == 3 and D == pytest.approx([2.0, 3.0], rel=1e-12) and slope == pytest.approx([8.0 / math.pi, 0.0])
    D, slope, k = rw.directivity([[1.0, 0.25]], (0.0, 0.0, -2.0), (0.0, 0.0, 1.0))
    assert k == 0 and D == pytest.approx([0.25], rel=1e-12)
    assert rw.directivity([[1.0, 0.25]], (0.0, 0.0, -2.0), (1.0, 0.0, 0.0))[0] == pytest.approx([0.625], rel=1e-12)


def test_emission_direction_by_hand():
    """the first hit-made node's ray, however many duplicate nodes lie before it; the connection's direction while the walk has
    not left the source, with the error (bounds + 2e-4) / length"""
    F0 = rw.Node((0.0, 0.0, 0.0), None, None, 1.0)
    dup = rw.Node(F0.pos, None, None, 0.07)
    hit = rw.Node((0.0, 100.0, 0.0), (0.0, -1.0, 0.0), 0, 0.07, 1e-3, arrive=(0.0, 1.0, 0.0))
    later = rw.Node((50.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0, 0.2, 2e-3, arrive=(0.6, -0.8, 0.0))
    B = rw.Node((300.0, 0.0, 400.0), (0.0, 0.0, -1.0), 0, 0.2, 3e-3)
    assert rw.emission([F0, dup, hit, later], B) == ((0.0, 1.0, 0.0), rw.WALK_RAY_ERROR, True)
    assert rw.emission([F0, hit], B)[0] == (0.0, 1.0, 0.0)
    w, delta, walked = rw.emission([F0, dup, dup], B)
    assert w == pytest.approx((0.6, 0.0, 0.8)) and not walked and delta == pytest.approx((0.0 + 3e-3 + 2e-4) / 500.0)
    assert rw.emission([F0], B)[0] == pytest.approx((0.6, 0.0, 0.8))
    assert rw.order_of([F0, dup, hit, later], [B, B]) == 2


def test_a_plain_descriptor_is_the_frame():
    """no table, the whole window: the same terms in the same order, the frame's bits; an all-ones table likewise"""
    for mode in (None, "uniform"):
        fr = source_frame(mode, 4, 101, 256)
        for table in (None, np.ones((4, 5), np.float32)):
            a = rw.apply_source(fr, None if table is None else table.tolist(), OBLIQUE, rtol=rtol_of(mode))
            assert a.H == fr.H and a.count == fr.count and (a.deposits, a.steps, a.connections) == (fr.deposits, fr.steps, fr.connections)
            assert a.d_flagged == 0 and a.flagged == (fr.flagged if isinstance(fr.flagged, int) else len(fr.flagged))


# ---- directivity, pair by pair, against the restatement built from the oracle's pieces --------------------------------------------------------
def compare_directional(oracle_mod, osc, fr, mode, depth, seed, pairs, table, source=rw.SOURCE, orientation=OBLIQUE):
    """-> (largest relative difference of a (pair, band, bin) entry, pairs compared, pairs that disagree: another set of occupied
    bins or an entry beyond the tolerance).  A pair with a flagged contribution is not compared."""
    flags = MODES[mode][0] if mode else 0
    rtol = rtol_of(mode, True, depth)
    op = oracle_mod.default_params(num_pairs=pairs, depth=depth, seed=seed, russian_roulette=1, flags=flags)
    T = TABLES[table]
    worst, compared, wrong = 0.0, 0, 0
    for i in range(pairs):
        a = rw.apply_source(fr, T.tolist(), orientation, rtol=rtol, pair_range=(i, i + 1))
        if a.flagged:
            continue
        _, e64 = restate(oracle_mod, osc, op, source, rw.LISTENER, table=T, fwd=orientation, pairs=i + 1, pair_begin=i)
        H = np.asarray(a.H)
        compared += 1
        nz = H != 0.0
        if not np.array_equal(e64 != 0.0, nz):
            wrong += 1
            continue
        if nz.any():
            d = float(np.abs(e64[nz] / H[nz] - 1.0).max())
            wrong += d > rtol
            worst = max(worst, d)
    return worst, compared, wrong


DIRECTIONAL = [(None, 1024), ("uniform", 256), ("balance", 256), ("lobes", 256), ("lobes_all", 256)]


@pytest.mark.parametrize("depth", [4, 8])
@pytest.mark.parametrize("mode,pairs", DIRECTIONAL, ids=[m or "end_to_end" for m, _ in DIRECTIONAL])
def test_directional_frames_pair_by_pair(oracle_mod, mode, pairs, depth):
    """Per pair the model's directional deposits (rw.apply_source on the pair) against restate(..., pair_begin = i, pairs = i + 1) with
    the same table: the same occupied bins (deposited or not, the bin exactly) and every (band, bin) entry to the frame's tolerance.
    A pair with a flagged contribution — by the walk, the connection, MinSeg, a bin edge, a weight fallback, or D too steep for the
    direction's error — is not compared; at most 2 % of a frame's contributions may be flagged, and at least half its pairs are
    compared.  The all-prefix frames must take both kinds of emission direction: the walk's ray and the connection's.
    Measured (3 seeds x 3 tables each; flagged of which for D alone; the largest relative difference of an entry):

      frame                   contributions      flagged (for D alone)        largest difference, depth 4 / 8
      end to end, 1 024       1 024              2-19 (2-19) / 11-13 (8-10)   9.3e-6 / 5.3e-5
      uniform, 256            4 244-10 212       2-14 (0-12) / 15-106 (4-87)  5.4e-6 / 4.6e-5
      balance, 256            same               1-6 (0-4) / 6-75 (1-28)      9.0e-6 / 5.1e-5
      lobes, 256              256                0-3 / 0-5                    5.5e-6 / 1.7e-5
      lobes_all, 256          same as uniform    8-39 (2-31) / 65-153         5.5e-6 / 1.3e-5

    Every figure but one lies within a quarter of its mode's tolerance, which therefore stands for the directional frames too.  End to
    end at depth 8 the 5.3e-5 (seed 101) is no matter of D: the same pair differs by 5.2e-5 without a table — ENERGY_RTOL was measured
    on frames of depth 1, 2 and 4.  DIRECTIONAL_RTOL of tests/test_independent_restatement.py holds 4 x that figure for (end to end,
    depth 8); no GPU test uses such a frame.
    Deliberate errors made in the model (not committed), depth 4, seed 101, the cardioid / the two-sample table; pairs that then disagree
    among those compared, beside the frame's flagged contributions:

      error                                                 end to end, 1 024 pairs      uniform, 256 pairs       flagged
      none                                                  0 / 0                        0 / 0                    19 / 2, 6 / 2
      the first hit among F1..F(i+1) instead of F1..Fi      0 / 0 (no prefixes)          81 / 85                  same
      k + 1 for k in the lerp                               634 / 0 (K = 2: k is 0)      215 / 0                  same
      theta = acos(w . f), f not normalised                 592 / 421                    132 / 29                 same
      the ray of step 0 whether it hit or not               0 / 0                        0 / 0                    same

    The last line is why test_directional_frames_whose_first_steps_miss exists."""
    sc, osc = mode_scene(oracle_mod, mode) if mode else model_scene(oracle_mod)
    worst_all = 0.0
    for seed in SEEDS:
        fr = source_frame(mode, depth, seed, pairs)
        for table in tables_of(mode, depth):
            a, rtol = applied(fr, mode, table, depth=depth)
            worst, compared, wrong = compare_directional(oracle_mod, osc, fr, mode, depth, seed, pairs, table)
            worst_all = max(worst_all, worst)
            print(f"{mode} depth {depth} seed {seed} {table}: flagged {a.flagged} (for D alone {a.d_flagged}) of {a.connections} deposits {a.deposits} "
                  f"walk ray {a.walk_ray} connection ray {a.connection_ray} pairs compared {compared} disagreeing {wrong} worst {worst:.3e}")
            assert wrong == 0
            assert a.flagged <= 0.02 * a.connections
            assert compared >= pairs // 2 and a.deposits > pairs // 10
            if mode in ("uniform", "balance", "lobes_all"):
                assert a.connection_ray > pairs // 4 and a.walk_ray > pairs      # both sources of the direction are exercised
    print(f"{mode} depth {depth}: largest relative difference {worst_all:.3e}, tolerance {rtol_of(mode, True, depth):.3e}")
    if (mode, depth) not in DIRECTIONAL_RTOL:
        assert worst_all <= 0.25 * rtol_of(mode)       # else the mode needs an entry of its own in DIRECTIONAL_RTOL


@pytest.mark.parametrize("mode,pairs", DIRECTIONAL[:2], ids=["end_to_end", "uniform"])
def test_directional_frames_whose_first_steps_miss(oracle_mod, mode, pairs):
    """From rw.SOURCE no FIRST step of a walk misses (the slab and the side walls cover the open x = 3000 side: 0 of 1 024 walks),
    so the frames above cannot tell "the ray of the first step that HIT" from "the ray of step 0".  From (2000, 300, 150), beyond the
    slab, 53 of 1 024 (15 of 256) source walks miss at step 0 and 49 (15) of them hit something later: depth 4, seed 101, the cardioid
    and the two-sample table, facing (-1, 0.2, 0.1).
    Measured: no compared pair disagrees, largest relative difference 4.6e-6; 16 / 3 flagged of 1 024 end to end, 9 / 1 of 4 323 with
    all prefixes.  With the ray of step 0 taken whether it hit or not, 45 / 46 of some 1 010 pairs disagree end to end and 15 / 15 of
    some 250 with all prefixes; with the first hit among F1..F(i+1), 219 / 226 of the latter."""
    sc, osc = mode_scene(oracle_mod, mode) if mode else model_scene(oracle_mod)
    fr = source_frame(mode, 4, 101, pairs, source=SOURCES[2])
    missed_first = sum(1 for r in fr.pairs if len(r.fwd) > 1 and r.fwd[1].arrive is None)
    hit_later = sum(1 for r in fr.pairs if len(r.fwd) > 1 and r.fwd[1].arrive is None and any(n.arrive is not None for n in r.fwd))
    assert missed_first >= pairs // 20 and hit_later >= pairs // 50, (missed_first, hit_later)
    # (end to end the cardioid on its floor of 0.02 leaves out 23 of 1 024 for D alone, past the cap: the raised floor, see RAISED)
    for table in ("cardioid_raised" if mode is None else "cardioid", "two"):
        a, rtol = applied(fr, mode, table, (-1.0, 0.2, 0.1))
        worst, compared, wrong = compare_directional(oracle_mod, osc, fr, mode, 4, 101, pairs, table, SOURCES[2], (-1.0, 0.2, 0.1))
        print(f"{mode} from {SOURCES[2]} {table}: first steps missed {missed_first} (hit later {hit_later}) flagged {a.flagged} (for D alone "
              f"{a.d_flagged}) of {a.connections} deposits {a.deposits} pairs compared {compared} disagreeing {wrong} worst {worst:.3e}")
        assert wrong == 0 and a.flagged <= 0.02 * a.connections
        assert compared >= pairs // 2 and a.deposits > pairs // 10
        assert worst <= 0.25 * rtol_of(mode)


# ---- ignored actors, pair by pair, against the oracle ---------------------------------------------------------------------------------------
def box_oracle(oracle_mod, sc, cut=1, lobes=False):
    tri, mat = sc.triangles(cut)
    osc = oracle_mod.Scene(np.asarray(tri, np.float32), np.asarray(mat, np.uint16), np.asarray(sc.absorption, np.float32),
                           transmission=LOBE_TAU if lobes else None, scattering=LOBE_SIGMA if lobes else None)
    osc.set_objects(np.asarray(sc.object_ids(cut), np.uint32))
    return osc


def compare_ignored(oracle_mod, osc, fr, mode, depth, seed, pairs):
    """compare_mode_frame of tests/test_independent_restatement.py with the two ignored actors in the oracle's parameters, counting
    -> (largest relative difference, pairs compared, pairs that disagree, the oracle's deposits in all pairs)"""
    flags = MODES[mode][0] if mode else 0
    rtol = rtol_of(mode)
    p = oracle_mod.default_params(num_pairs=pairs, depth=depth, seed=seed, russian_roulette=1, flags=flags, source_object=BOX_ACTOR,
                                  listener_object=SLAB_ACTOR)
    prefix = isinstance(fr, rw.PrefixFrame)
    worst, compared, wrong, deposits = 0.0, 0, 0, 0
    for i, r in enumerate(fr.pairs):
        e32, e64, cnt = osc.compute_energy(p, rw.SOURCE, rw.LISTENER, pair_begin=i, pair_end=i + 1)
        deposits += cnt.deposits
        assert cnt.closest_rays == r.steps and cnt.path_nodes == len(r.fwd) + len(r.bwd), (seed, i)      # the roulette is exact
        assert cnt.any_rays == (r.connections if prefix else 1), (seed, i)
        a = rw.apply_source(fr, pair_range=(i, i + 1))
        if a.flagged:
            continue
        compared += 1
        H = np.asarray(a.H)
        nz = H != 0.0
        if cnt.deposits != a.deposits or not np.array_equal(e64 != 0.0, nz):
            wrong += 1
            continue
        if nz.any():
            d = float(np.abs(e64[nz] / H[nz] - 1.0).max())
            wrong += d > rtol
            worst = max(worst, d)
    return worst, compared, wrong, deposits


IGNORED = [(None, 1024), ("uniform", 256), ("lobes", 1024)]


@pytest.mark.parametrize("mode,pairs", IGNORED, ids=[m or "end_to_end" for m, _ in IGNORED])
def test_ignored_actors_pair_by_pair(oracle_mod, mode, pairs):
    """The box scene at depth 4, walls cut 1 x 1 (seeds 101, 202) and 4 x 4 (seed 101): per pair the step, node and connection
    counters exactly (flagged pairs too), and for a pair without a flagged contribution the deposit count, the occupied bins and
    every (band, bin) entry.  The largest difference must stay within a QUARTER of the mode's tolerance: only which rectangles a
    walk sees changes, the evaluation does not, so ENERGY_RTOL / mode_rtol hold for these frames as they stand.
    Measured (seed 101 / 202; the cut changes no figure):

      end to end, 1 024 pairs    flagged 0 / 1, deposits model 646 / 648, oracle 646 / 649, largest difference 3.5e-6 / 7.3e-6
      uniform, 256 pairs         flagged 3 of 4 323 / 2 of 4 244, deposits 1 989 / 1 875, oracle 1 990 / 1 877, 2.7e-6 / 4.1e-6
      lobes, 1 024 pairs         flagged 0 / 2, deposits 610 / 621, oracle 610 / 622, 6.0e-6 / 2.3e-6; lobes picked 797 / 676 / 1 154

    A deliberate error made in the model (not committed): the listener's walks ignoring the SOURCE'S actor (7) instead of their own
    makes 126 of 1 024 pairs disagree end to end and 38 of 253 with all prefixes (0 and 3 contributions flagged)."""
    lobes = mode == "lobes"
    for cut in (1, 4):
        osc = box_oracle(oracle_mod, box_scene(), cut, lobes)
        for seed in SEEDS[:2] if cut == 1 else SEEDS[:1]:
            fr = source_frame(mode, 4, seed, pairs, box=True)
            nfr = fr.flagged if isinstance(fr.flagged, int) else len(fr.flagged)
            worst, compared, wrong, deposits = compare_ignored(oracle_mod, osc, fr, mode, 4, seed, pairs)
            print(f"{mode} cut {cut} seed {seed}: flagged {nfr} of {fr.connections} deposits {fr.deposits} / {deposits} pairs compared {compared} "
                  f"disagreeing {wrong} worst {worst:.3e} lobes {fr.lobes}")
            assert wrong == 0
            assert nfr <= 0.02 * fr.connections and fr.deposits > pairs // 10
            assert abs(deposits - fr.deposits) <= nfr
            assert worst <= 0.25 * rtol_of(mode)       # the evaluation does not change: the mode's tolerance holds as it stands
            if lobes:
                assert min(fr.lobes) >= 100


class LeakyScene(rw.Scene):
    """a DELIBERATE error for a control: the connection's query ignores the two actors as well"""

    def any_hit(self, *args, **kw):
        return rw.Scene([r for r in self.rects if r.object not in (BOX_ACTOR, SLAB_ACTOR)], self.absorption).any_hit(*args, **kw)


def test_ignored_actor_controls():
    """on the model alone.  Nothing ignored: the source is sealed in its box and the frame deposits nothing.  The connection
    ignoring the actors too: far more deposits than the flagged contributions could explain — the asymmetry of the rule (the walks
    ignore their own actor, ConnectSubpaths ignores nothing) is exercised by the frames."""
    for mode, pairs in ((None, 1024), ("uniform", 256)):
        sealed = source_frame(mode, 4, 101, pairs, box=True, ignore=(rw.NO_OBJECT, rw.NO_OBJECT))
        assert sealed.deposits == 0 and not np.asarray(sealed.H).any()
        fr = source_frame(mode, 4, 101, pairs, box=True)
        sc = box_scene()
        leaky = LeakyScene(sc.rects, sc.absorption)
        prm = rw.Params(bands=4, seed=101, depth=4, axis_bounds=mode is not None)
        if mode:
            wrong = rw.PrefixFrame(leaky, prm, rw.SOURCE, rw.LISTENER, pairs, ignore=(BOX_ACTOR, SLAB_ACTOR))
        else:
            wrong = rw.Frame(leaky, prm, rw.SOURCE, rw.LISTENER, pairs, ignore=(BOX_ACTOR, SLAB_ACTOR))
        nfr = fr.flagged if isinstance(fr.flagged, int) else len(fr.flagged)
        print(f"{mode}: deposits {fr.deposits}, with a connection that ignores too {wrong.deposits}, flagged {nfr}")
        assert wrong.steps == fr.steps
        assert wrong.deposits > fr.deposits + 10 * max(nfr, 1) + pairs // 10
        # the listener's walks do pass through the slab, the source's leave the box: nodes that only an ignoring walk can make
        assert fr.steps > sealed.steps or fr.deposits > 0
