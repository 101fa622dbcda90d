"""An INDEPENDENT float64 restatement of the path — written from the reference's lines, not from oracle/fs_oracle.c —
checked against the C oracle on thousands of random inputs.  The closed-form pieces:

  EvaluatePath                 Private/AudioRayTracingSubsystem.cpp:358-420
  AddEnergyAtDelay (bin rule)  Public/FrequenSeeAudioComponent.h:87-91
  ReconstructImpulseResponse   Private/FrequenSeeAudioComponent.cpp:320-380 (+ NormalizeImpulseResponse :382-406)

and, with the model of tests/restate_walk.py (axis-aligned rectangles intersected analytically, every discrete decision
with a margin), the walk and the connection:

  GeneratePath                 Private/AudioRayTracingSubsystem.cpp:279-355   step by step on uncapped walks
  ConnectSubpaths              Private/AudioRayTracingSubsystem.cpp:235-277   verdicts; node order through whole pairs

and the three modes the build owns (FS_FLAG_ALL_CONNECTIONS, FS_FLAG_MIS_BALANCE, FS_FLAG_MATERIAL_LOBES), which the model restates
from include/frequensee.h and DESIGN.md section 8: whole frames, pair by pair, every contribution (i, j) with its own flag.

The reference ships no golden vectors for this path ("parity unpinned"): what pins the oracle is hand-derived KATs
(tests/test_oracle_kat.py) and this second, differently written implementation — two restatements that agree on
random data are much less likely to share a misreading than one is to contain it.  The oracle computes in fp32 like
the reference, this file in float64: agreement is asserted to fp32 accuracy, bins exactly (away from bin edges).
"""
import math

import numpy as np
import pytest

import restate_walk as rw
from restate_walk import bin_of

NUM_BINS = 1000            # FSAC.h:137
SAMPLE_RATE = 48000        # FSAC.h:133


def evaluate_path_f64(positions, reflectivity, has_material, probability):
    """ARTS.cpp:358-420 for one path and one band (tests/restate_walk.py holds the lines, for any number of bands): positions
    [n][3] (cm), per node: Absorption[2] value, whether the node has a geometry component with a material, and its Probability.
    Returns (DelaySeconds, Gain)."""
    delay, gains, _ = rw.evaluate_path_bands_f64(positions, [[r] for r in reflectivity], has_material, probability)
    return delay, gains[0]


def reconstruct_f64(energy, num_samples=SAMPLE_RATE, samples_per_bin=49):
    """FSAC.cpp:320-380.  NumSamplesPerBin = CeilToInt(0.001f * 48000) = 49 in float32 arithmetic (0.001f * 48000 =
    48.000004f); EnergyResponse and EnergyNorms alias the same buffer (:325, :329); NormalizeImpulseResponse zeroes the
    UNFILTERED array, which is then replaced by the filtered one (:377-378) — the result is the filtered signal."""
    energy = np.asarray(energy, dtype=np.float64)
    pi4 = math.sqrt(4.0 * math.pi)                                          # :323
    amp = np.zeros_like(energy)
    ok = np.abs(energy) >= 1e-6                                             # :343
    amp[ok] = energy[ok] / np.sqrt(energy[ok] * pi4)                        # :345
    ir = np.zeros(num_samples)
    for b in range(len(energy)):
        prev = amp[b] if b == 0 else amp[b - 1]                             # :347-355
        n = min(samples_per_bin, num_samples - b * samples_per_bin)         # :340
        for k in range(max(n, 0)):
            w = k / samples_per_bin                                         # :359
            ir[b * samples_per_bin + k] = (1.0 - w) * prev + w * amp[b]     # :360-362
    out = np.empty_like(ir)
    out[0] = ir[0]                                                          # :371
    for i in range(1, num_samples):
        out[i] = 0.25 * ir[i] + 0.75 * out[i - 1]                           # :372-375
    return out


def random_path(rng, oracle_mod):
    n = int(rng.integers(2, 19))
    scale = float(rng.choice([300.0, 1500.0, 4000.0, 12000.0]))            # short hops (skipped) and long ones
    pos = np.cumsum(rng.normal(size=(n, 3)) * scale, axis=0).astype(np.float32)
    has = rng.random(n) < 0.8
    mat = np.where(has, rng.integers(0, 4, size=n), oracle_mod.NO_MATERIAL)
    prob = np.where(rng.random(n) < 0.1, 1.0, rng.uniform(1e-3, 0.3, size=n)).astype(np.float32)
    nodes = [oracle_mod.make_node(pos[i], material=int(mat[i]), prob=float(prob[i])) for i in range(n)]
    return nodes, pos.astype(np.float64), has, mat, prob.astype(np.float64)


def test_evaluate_path_and_bin_rule_against_float64(oracle_mod):
    rng = np.random.default_rng(20250101)
    refl = rng.uniform(0.05, 0.9, size=(4, 1)).astype(np.float32)           # 4 materials, 1 band (slot 0 == Absorption[2])
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)         # EvaluatePath never touches the geometry
    osc = oracle_mod.Scene(tri, np.zeros(1, np.uint16), refl)
    p = oracle_mod.default_params(num_pairs=1, depth=0)
    checked = edge = clamped = 0
    for _ in range(4000):
        nodes, pos, has, mat, prob = random_path(rng, oracle_mod)
        gains, delay = osc.evaluate_path(p, nodes)
        r = [float(refl[int(m), 0]) if h else 0.0 for m, h in zip(mat, has)]
        want_delay, want_gain = evaluate_path_f64(pos, r, has, prob)
        assert delay == pytest.approx(want_delay, rel=2e-6, abs=1e-12)
        assert float(gains[0]) == pytest.approx(want_gain, rel=3e-5, abs=1e-30)
        clamped += want_gain == 10.0
        x = want_delay * 1000.0
        if abs(x - round(x)) < 1e-5 * max(abs(x), 1.0):
            edge += 1                                                       # a bin edge within fp32 noise: either side is right
            continue
        buf = np.zeros(NUM_BINS, np.float32)
        assert oracle_mod.add_energy_at_delay(buf, delay, 1.0) == bin_of(want_delay)
        checked += 1
    assert checked > 3900 and edge < 100 and clamped > 50                                  # both branches of the clamp were exercised
    # the clamp ends of the bin rule (FSAC.h:89)
    buf = np.zeros(NUM_BINS, np.float32)
    for d, b in ((-0.5, 0), (0.0, 0), (0.0004, 0), (0.9995, 999), (1.7, 999), (0.0145772595, 14)):
        assert oracle_mod.add_energy_at_delay(buf, d, 1.0) == b == bin_of(d)


def test_reconstruct_against_float64(oracle_mod):
    rng = np.random.default_rng(7)
    for trial in range(12):
        e = np.zeros(NUM_BINS, np.float32)
        k = int(rng.integers(1, 400))
        idx = rng.integers(0, NUM_BINS, size=k)
        e[idx] = (10.0 ** rng.uniform(-8, 0.5, size=k)).astype(np.float32)  # straddles the 1e-6 threshold
        got = oracle_mod.reconstruct(e)
        want = reconstruct_f64(e)
        peak = np.abs(want).max()
        assert peak > 0
        assert np.abs(got - want).max() <= 2e-6 * peak
        assert np.array_equal(got[980 * 49:] != 0, want[980 * 49:] != 0)    # bins >= 980 write nothing, the filter tail decays
    assert reconstruct_f64(np.zeros(NUM_BINS)).max() == 0.0


# ---- GeneratePath and ConnectSubpaths: the model of tests/restate_walk.py against the oracle ------------------------------------------
ENERGY_RTOL = 4e-5     # 4 x the largest relative difference test_whole_pairs_against_the_model measures (see there)


def model_scene(oracle_mod, cut=1):
    """(the model's scene, the oracle's scene of the same rectangles cut into cut x cut cells of two triangles)"""
    sc = rw.make_test_scene()
    tri, mat = sc.triangles(cut)
    return sc, oracle_mod.Scene(np.asarray(tri, np.float32), np.asarray(mat, np.uint16), np.asarray(sc.absorption, np.float32))


def model_node(nd, oracle_mod):
    """an oracle node as the model's state: float32 values taken as they are, zero signs included"""
    nrm = tuple(float(x) for x in nd.normal)
    return rw.Node(tuple(float(x) for x in nd.pos), None if nrm == (0.0, 0.0, 0.0) else nrm,
                   rw.NO_MATERIAL if nd.material == oracle_mod.NO_MATERIAL else int(nd.material), float(nd.prob))


def same_float(a, b):
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


def test_philox_words_are_the_only_common_input(oracle_mod):
    """the model's Philox4x32-10, written out in Python, gives the oracle's words and uniforms"""
    import ctypes as C
    lib = oracle_mod.load()
    rng = np.random.default_rng(11)
    cases = [((0, 0, 0, 0), (0, 0)), ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2), ((7, 3, 0, 0x46533031), (0x5EED, 0))]
    cases += [(tuple(int(x) for x in rng.integers(0, 2 ** 32, 4)), tuple(int(x) for x in rng.integers(0, 2 ** 32, 2))) for _ in range(500)]
    for ctr, key in cases:
        out = (C.c_uint32 * 4)()
        lib.fso_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert tuple(out) == rw.philox4x32_10(ctr, key)
        assert all(float(lib.fso_u01(w)) == rw.u01(w) for w in out)
    assert rw.draw(0x123456789, 5, 1, 3, 2) == rw.philox4x32_10((5, 7, 2, 0x46533031), (0x23456789, 0x1))


_uncapped = {}


def uncapped_walks(oracle_mod):
    """the oracle's walks of 2048 pairs, both sides, depth = 0 and the default roulette: {(pair, side): nodes}"""
    if not _uncapped:
        sc, osc = model_scene(oracle_mod)
        p = oracle_mod.default_params(num_pairs=2048, depth=0, seed=0xC0FFEE)
        for i in range(2048):
            for side, start in ((0, rw.SOURCE), (1, rw.LISTENER)):
                nodes = osc.generate_path(p, i, side, start, max_nodes=1024)
                assert len(nodes) < 1024
                _uncapped[(i, side)] = nodes
        _uncapped["scene"] = (sc, osc, p)
    return _uncapped


def test_walk_step_by_step_uncapped(oracle_mod):
    """GeneratePath (ARTS.cpp:279-355), uncapped, 2 x 2048 walks of up to 100 and more nodes.  float32 and float64 walks drift
    apart with depth (grazing bounces amplify the in-plane error by 1 / cos), so the comparison is step by step: from the
    ORACLE's node k the model takes one turn of the loop in float64 and must arrive at the oracle's node k + 1 — position to
    1e-3 cm, normal exactly (zero signs included), material exactly, probability to 2e-6 relative — and the model's roulette must
    end the walk exactly where the oracle's walk ends.  Turns with a fragile decision are skipped.
    Measured: 37 556 turns, none flagged, 3 090 misses, 3 walks of more than 64 nodes; worst position difference 6.2e-4 cm,
    worst probability difference 2.3e-7."""
    walks = uncapped_walks(oracle_mod)
    sc, osc, p = walks["scene"]
    prm = rw.Params(bands=4, seed=p.seed, depth=0)
    steps = flagged = misses = long_walks = slab = bare = 0
    worst_pos = worst_prob = 0.0
    for (i, side), nodes in ((k, v) for k, v in walks.items() if k != "scene"):
        long_walks += len(nodes) > 64
        for k, nd in enumerate(nodes):
            got = rw.step(sc, prm, i, side, k, model_node(nd, oracle_mod))
            if k == len(nodes) - 1:
                assert got is None, (i, side, k)                     # the roulette ends the walk here and nowhere else
                break
            assert got is not None, (i, side, k)
            node, fragile, hit = got
            steps += 1
            if fragile:
                flagged += 1
                continue
            want = model_node(nodes[k + 1], oracle_mod)
            misses += not hit
            slab += hit and node.material == 1
            bare += hit and node.material is rw.NO_MATERIAL
            if not hit:                                              # the duplicate node: same place, new probability
                assert want.pos == model_node(nd, oracle_mod).pos and nodes[k + 1].material == nd.material
            assert math.dist(node.pos, want.pos) <= 1e-3, (i, side, k, node.pos, want.pos)
            assert (node.normal is None) == (want.normal is None), (i, side, k)
            if node.normal is not None:
                assert all(same_float(a, b) for a, b in zip(node.normal, want.normal)), (i, side, k, node.normal, want.normal)
            assert node.material == want.material, (i, side, k)
            assert node.prob == pytest.approx(want.prob, rel=2e-6), (i, side, k)
            worst_pos = max(worst_pos, math.dist(node.pos, want.pos))
            worst_prob = max(worst_prob, abs(node.prob / want.prob - 1.0))
    print(f"steps {steps} flagged {flagged} ({flagged / steps:.3%}) misses {misses} walks over 64 nodes {long_walks} slab hits {slab} "
          f"hits without material {bare} worst position {worst_pos:.3e} cm worst probability {worst_prob:.3e}")
    assert flagged <= 0.005 * steps
    assert misses > 100 and long_walks > 0 and slab > 100 and bare > 100


def test_connection_verdicts(oracle_mod):
    """ConnectSubpaths' trace (ARTS.cpp:252-254: visible iff nothing is hit up to 0.1 cm before B) on the end nodes of all 2048
    uncapped pairs, on 4096 random (source-walk node, listener-walk node) pairs and on some 500 pairs whose second node lies just
    behind a face of the slab: the oracle's verdict equals the model's except where the model calls it fragile.  Measured: 0.15 % fragile, 58 % visible, 262 visible only because of the pull-back."""
    walks = uncapped_walks(oracle_mod)
    sc, osc, p = walks["scene"]
    prm = rw.Params(bands=4)
    rng = np.random.default_rng(5)
    cases = [(walks[(i, 0)][-1], walks[(i, 1)][-1]) for i in range(2048)]
    for _ in range(4096):
        f, b = walks[(int(rng.integers(2048)), 0)], walks[(int(rng.integers(2048)), 1)]
        cases.append((f[int(rng.integers(len(f)))], b[int(rng.integers(len(b)))]))
    # Between nodes that sit 0.1 cm off their walls the pull-back (0.1 cm, :253) never decides.  Here it does: B lies 0.02 ... 0.3 cm
    # BEHIND a face of the slab as seen from F, so that face is the last thing before B — inside the pull-back or just outside it
    for _ in range(600):
        f = walks[(int(rng.integers(2048)), 0)]
        f = f[int(rng.integers(len(f)))]
        if 1390.0 <= f.pos[0] <= 1510.0:
            continue
        x = 1400.0 + float(rng.choice([0.02, 0.05, 0.07, 0.15, 0.3])) if f.pos[0] < 1400.0 else 1500.0 - float(rng.choice([0.02, 0.05, 0.07, 0.15, 0.3]))
        cases.append((f, oracle_mod.make_node((x, rng.uniform(350.0, 1250.0), rng.uniform(150.0, 650.0)))))
    fragile = visible = by_pullback = 0
    no_pullback = rw.Params(bands=4, connect_pullback=0.0)
    for f, b in cases:
        want, fr = rw.connect(sc, prm, model_node(f, oracle_mod), model_node(b, oracle_mod))
        if fr:
            fragile += 1
            continue
        assert osc.connect(p, f, b) == want, (list(f.pos), list(b.pos))
        visible += want
        by_pullback += want and not rw.connect(sc, no_pullback, model_node(f, oracle_mod), model_node(b, oracle_mod))[0]
    assert by_pullback > 50, by_pullback
    n = len(cases) - fragile
    print(f"connections {len(cases)} visible only by the pull-back {by_pullback} fragile {fragile} ({fragile / len(cases):.3%}) visible {visible / n:.3%}")
    assert fragile <= 0.02 * len(cases)
    assert 0.2 * n <= visible <= 0.8 * n


_frames = {}


def model_frame(depth, roulette, cosine, seed, num_pairs=1024, gain=10.0, keep_pairs=False):
    """the model's frame of the test scene, cached: the GPU tests (tests/test_gpu_restatement.py) share them"""
    key = (depth, roulette, cosine, seed, num_pairs, gain)
    if key not in _frames or (keep_pairs and not _frames[key].pairs):
        prm = rw.Params(bands=4, seed=seed, depth=depth, russian_roulette=roulette, cosine=cosine, energy_gain=gain)
        _frames[key] = rw.Frame(rw.make_test_scene(), prm, rw.SOURCE, rw.LISTENER, num_pairs, keep_pairs=keep_pairs)
    return _frames[key]


@pytest.mark.parametrize("cosine", [False, True], ids=["cone", "cosine"])
@pytest.mark.parametrize("roulette", [True, False], ids=["rr", "norr"])
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_whole_pairs_against_the_model(oracle_mod, depth, roulette, cosine):
    """Frames of 1024 pairs, 3 seeds: pair by pair the oracle's compute_energy(pair_begin = i, pair_end = i + 1) against the
    model's deposit — deposited or not (the `deposits` counter), the bin exactly, the energy of every band to ENERGY_RTOL —
    and the node counts of both walks.  Every pair the model does not flag must agree; at most 2 % may be flagged.  The
    distance between the oracle's and the model's last nodes must stay below the model's running bound.
    Measured over the 36 frames: largest relative energy difference 9.9e-6 at depth 4 (1.0e-6 at depth 1, 4.9e-6 at depth 2;
    ENERGY_RTOL = 4 x the largest), largest end-point difference 0.46 of the bound, 0 ... 0.3 % of a frame's pairs flagged
    (depth 1: none, depth 2: up to 0.1 %, depth 4: up to 0.3 %)."""
    sc, osc = model_scene(oracle_mod)
    B = 4
    worst_e = worst_ratio = 0.0
    for seed in (101, 202, 303):
        fr = model_frame(depth, roulette, cosine, seed, keep_pairs=True)
        p = oracle_mod.default_params(num_pairs=1024, depth=depth, seed=seed, russian_roulette=int(roulette),
                                      flags=oracle_mod.FLAG_COSINE_SAMPLING if cosine else 0)
        steps = 0
        for i, r in enumerate(fr.pairs):
            e32, e64, cnt = osc.compute_energy(p, rw.SOURCE, rw.LISTENER, pair_begin=i, pair_end=i + 1)
            steps += cnt.closest_rays
            assert cnt.path_nodes == len(r.fwd) + len(r.bwd), (seed, i)       # the roulette is exact: flagged pairs too
            if r.fragile:
                continue
            assert cnt.deposits == int(r.visible), (seed, i)
            for side, (start, mine) in enumerate(((rw.SOURCE, r.fwd), (rw.LISTENER, r.bwd))):
                end = osc.generate_path(p, i, side, start)[-1]
                if mine[-1].bound > 0.0:
                    worst_ratio = max(worst_ratio, math.dist(mine[-1].pos, [float(x) for x in end.pos]) / mine[-1].bound)
            if not r.visible:
                assert not e64.any()
                continue
            for b in range(B):
                assert np.flatnonzero(e64[b]).tolist() == [r.bin], (seed, i, b)
                d = abs(e64[b][r.bin] / r.energy[b] - 1.0)
                worst_e = max(worst_e, d)
                assert d <= ENERGY_RTOL, (seed, i, b, d)
        assert steps == fr.steps
        print(f"depth {depth} roulette {roulette} cosine {cosine} seed {seed}: flagged {len(fr.flagged) / 1024:.2%} "
              f"deposits {fr.deposits} worst energy {worst_e:.3e} worst end-point / bound {worst_ratio:.3f}")
        assert len(fr.flagged) <= 0.02 * 1024
        assert 100 < fr.deposits < 900
    assert worst_ratio < 1.0


# ---- the build-owned modes: all prefixes, balance-heuristic weights, lobes in the walk -------------------------------------------------------
# Transmission / Scattering of the test scene's two materials (its Absorption: 0.85 0.7 0.55 0.4 / 0.3 0.45 0.6 0.75).  Lobe
# probabilities (diffuse, specular, transmitted): 0.289 0.267 0.444 and 0.316 0.297 0.387, all >= 0.2; material 1 has tau = 0.5 >
# alpha = 0.3 in band 0, where the clamp Refl + tau <= 1 cuts it to 0.3
LOBE_TAU = [[0.3, 0.3, 0.3, 0.3], [0.5, 0.4, 0.3, 0.2]]
LOBE_SIGMA = [[0.4, 0.5, 0.6, 0.5], [0.6, 0.5, 0.4, 0.5]]

ALLC, MIS, LOBES, COSINE = 16, 32, 64, 4       # FS_FLAG_ALL_CONNECTIONS, _MIS_BALANCE, _MATERIAL_LOBES, _COSINE_SAMPLING
# mode -> (flags, 4 x the largest relative difference per (pair, band, bin) between oracle and model that test_mode_frames_against_
# _the_model and test_unbounded_depth_against_the_model measure over their frames on the CPU, see the former's docstring)
MODES = {
    "uniform": (ALLC, 3.0e-4),             # 7.65e-5: depth 8, seed 303
    "balance": (MIS, 6.9e-4),              # 1.73e-4: depth 8, seed 202
    "lobes": (LOBES, 1.2e-3),              # 3.11e-4: depth 8 without roulette, seed 101
    "lobes_all": (LOBES | ALLC, 1.1e-4),   # 2.96e-5: depth 8, seed 303
    "lobes_cosine": (LOBES | COSINE, 2.3e-4),   # 5.89e-5: depth 8, seed 202
}

# (mode (None: end to end), depth) -> the tolerance of its frames with a directivity table, where the mode's own does not do: 4 x the
# largest relative difference per (pair, band, bin) between the model and the oracle-built restatement with a table that
# tests/test_restatement_sources.py measures on the CPU (a mode and depth without an entry stayed within a quarter of its tolerance)
DIRECTIONAL_RTOL = {
    (None, 8): 2.2e-4,     # 5.28e-5: end to end, depth 8, 1 024 pairs, seed 101, the two-sample table (5.2e-5 without a table)
}


def mode_rtol(mode):
    return MODES[mode][1]


def mode_scene(oracle_mod, mode, cut=1):
    """(the model's scene, the oracle's) with the lobe arrays where the mode has them"""
    sc = rw.make_test_scene()
    tri, mat = sc.triangles(cut)
    lobes = bool(MODES[mode][0] & LOBES)
    if lobes:
        sc.set_lobes(LOBE_TAU, LOBE_SIGMA)
    return sc, oracle_mod.Scene(np.asarray(tri, np.float32), np.asarray(mat, np.uint16), np.asarray(sc.absorption, np.float32),
                                transmission=LOBE_TAU if lobes else None, scattering=LOBE_SIGMA if lobes else None)


_mode_frames = {}


def mode_frame(mode, depth, roulette, seed, num_pairs=1024, gain=10.0, keep_pairs=False, bands=4):
    """the model's frame of the test scene in one of MODES, cached: the GPU tests share them.  All-prefix modes give a
    rw.PrefixFrame, the end-to-end lobe modes a rw.Frame; both have H, count, deposits, steps, connections, lobes.  bands: the
    first so many of the scene's four (the lobe probabilities are band means: fewer bands are another walk)"""
    key = (mode, depth, roulette, seed, num_pairs, gain, bands)
    if key not in _mode_frames or (keep_pairs and not _mode_frames[key].pairs):
        flags = MODES[mode][0]
        sc = rw.make_test_scene()
        sc = rw.Scene(sc.rects, [row[:bands] for row in sc.absorption])
        if flags & LOBES:
            sc.set_lobes([row[:bands] for row in LOBE_TAU], [row[:bands] for row in LOBE_SIGMA])
        prm = rw.Params(bands=bands, seed=seed, depth=depth, russian_roulette=roulette, cosine=bool(flags & COSINE), lobes=bool(flags & LOBES),
                        energy_gain=gain, axis_bounds=True)
        if flags & (ALLC | MIS):
            fr = rw.PrefixFrame(sc, prm, rw.SOURCE, rw.LISTENER, num_pairs, balance=bool(flags & MIS), keep_pairs=keep_pairs)
        else:
            fr = rw.Frame(sc, prm, rw.SOURCE, rw.LISTENER, num_pairs, keep_pairs=keep_pairs)
        _mode_frames[key] = fr
    return _mode_frames[key]


def flagged_contributions(fr):
    return fr.flagged if isinstance(fr.flagged, int) else len(fr.flagged)      # (rw.PrefixFrame and rw.Applied count, rw.Frame lists)


def test_strategy_counts_by_hand():
    """N(t) = #{(i', j') in [0, D]^2, i' + j' = t}: t + 1 while the cap cuts nothing, 2 D - t + 1 beyond D, t + 1 for depth 0"""
    assert [rw.strategies(t, 2) for t in range(5)] == [1, 2, 3, 2, 1]
    assert [rw.strategies(t, 4) for t in range(9)] == [1, 2, 3, 4, 5, 4, 3, 2, 1]
    assert [rw.strategies(t, 8) for t in (0, 7, 8, 9, 16)] == [1, 8, 9, 8, 1]
    assert [rw.strategies(t, 0) for t in (0, 5, 8, 9, 100)] == [1, 6, 9, 10, 101]
    assert rw.strategy_range(5, 4) == (1, 4) and rw.strategy_range(3, 4) == (0, 3) and rw.strategy_range(9, 0) == (0, 9)
    for D in (1, 2, 5, 8):
        for t in range(2 * D + 1):
            assert rw.strategies(t, D) == sum(1 for i in range(D + 1) for j in range(D + 1) if i + j == t)


def test_lobe_table_by_hand():
    """alpha = 0.3, tau = 0.5, sigma = 0.6: Refl = 0.7, tau cut to 0.3, diffuse 0.42, specular 0.28, transmitted 0.3; the rows of the
    test's arrays; a material that reflects and transmits nothing keeps the diffuse lobe; the pick's intervals and margins"""
    sc = rw.make_test_scene()
    sc.set_lobes(LOBE_TAU, LOBE_SIGMA)
    g = sc.lobe_gain[1]
    assert [g[lobe][0] for lobe in range(3)] == pytest.approx([0.42, 0.28, 0.3], rel=1e-6)      # the clamp acts
    assert [g[lobe][3] for lobe in range(3)] == pytest.approx([0.125, 0.125, 0.2], rel=1e-6)    # and here it does not
    assert sc.lobe_prob[0] == pytest.approx([0.195 / 0.675, 0.18 / 0.675, 0.3 / 0.675], rel=1e-6)
    assert sc.lobe_prob[1] == pytest.approx([0.245 / 0.775, 0.23 / 0.775, 0.3 / 0.775], rel=1e-6)
    assert all(p >= 0.2 for row in sc.lobe_prob for p in row)
    for m in range(2):
        for b in range(4):
            assert sum(sc.lobe_gain[m][lobe][b] for lobe in range(3)) <= 1.0 + 1e-12
    dead = rw.Scene(sc.rects, [[1.0, 1.0]])
    dead.set_lobes([[0.0, 0.0]], [[0.5, 0.5]])
    assert dead.lobe_prob == [[1.0, 0.0, 0.0]] and dead.lobe_gain[0] == [[0.0, 0.0]] * 3
    pd, ps, pt = sc.lobe_prob[0]
    assert sc.pick_lobe(0, 0.0) == (rw.LOBE_DIFFUSE, pd, False) and sc.pick_lobe(0, pd + 0.5 * ps) == (rw.LOBE_SPECULAR, ps, False)
    assert sc.pick_lobe(0, 1.0 - 2.0 ** -24) == (rw.LOBE_TRANSMIT, pt, False)
    assert sc.pick_lobe(0, pd - 1e-7)[::2] == (rw.LOBE_DIFFUSE, True) and sc.pick_lobe(0, pd + ps + 1e-7)[::2] == (rw.LOBE_TRANSMIT, True)


def test_balance_weights_of_one_path_sum_to_one():
    """the model's weight alone: t = 1 by hand (floor z = -100, source (0, 0, 0), vertex (50, 0, -100), listener (200, 0, 0): p_1 =
    cos / (4 pi L0^2), p_0 = cos' / (4 pi L1^2), w_1 = L1^3 / (L0^3 + L1^3)); the weights of a path's strategies sum to 1 with and
    without the cap cutting strategies; both fallbacks"""
    up = (0.0, 0.0, 1.0)
    path = [rw.Node((0.0, 0.0, 0.0), None, None, 1.0), rw.Node((50.0, 0.0, -100.0), up, 0, 1.0), rw.Node((200.0, 0.0, 0.0), None, None, 1.0)]
    L0, L1 = math.sqrt(12500.0), math.sqrt(32500.0)
    w1 = L1 ** 3 / (L0 ** 3 + L1 ** 3)
    assert rw.balance_weight(path, 1, 8) == (pytest.approx(w1, rel=1e-14), None, False)
    assert rw.balance_weight(path, 0, 8)[0] == pytest.approx(1.0 - w1, rel=1e-14)
    assert rw.balance_weight(path, 1, 0)[0] == pytest.approx(w1, rel=1e-14)
    assert rw.balance_weight([path[0], path[2]], 0, 8) == (1.0, None, False)
    # a zigzag between floor z = 0 and ceiling z = 300: every vertex sees both neighbours, every strategy has a density
    zig = [rw.Node((0.0, 0.0, 100.0), None, None, 1.0)]
    for k in range(1, 7):
        zig.append(rw.Node((150.0 * k, 40.0 * k * k, 300.0 * (k % 2)), (0.0, 0.0, -1.0) if k % 2 else up, 0, 1.0))
    zig.append(rw.Node((1100.0, 500.0, 150.0), None, None, 1.0))
    for D in (0, 8, 6, 5, 4, 3):          # t = 6: D = 5, 4, 3 leave 5, 3, 1 of its 7 strategies
        lo, hi = rw.strategy_range(6, D)
        ws = [rw.balance_weight(zig, s, D) for s in range(lo, hi + 1)]
        assert len(ws) == rw.strategies(6, D) and all(w[1] is None and not w[2] and 0.0 < w[0] <= 1.0 for w in ws)
        assert sum(w[0] for w in ws) == pytest.approx(1.0, rel=1e-12)
    assert rw.balance_weight(zig, 3, 3)[0] == 1.0 and rw.balance_weight(zig, 3, 8)[0] < 0.9
    # the duplicate node of a missed step: the uniform weight; a segment of 1e-4 cm decides the same, but fragile
    dup = [path[0], path[1], rw.Node(path[1].pos, up, 0, 1.0), path[2]]
    assert rw.balance_weight(dup, 1, 8) == (1.0 / 3.0, "segment", False) and rw.balance_weight(dup, 1, 1) == (1.0, "segment", False)
    dup[2] = rw.Node((50.0, 0.00001, -100.0), up, 0, 1.0)
    assert rw.balance_weight(dup, 1, 8) == (1.0 / 3.0, "segment", True)
    # vertex 1 faces away from vertex 2: the forward walk cannot have left it that way, so strategy 2 has density 0 -> uniform
    back = [path[0], rw.Node((100.0, 0.0, -100.0), up, 0, 1.0), rw.Node((200.0, 0.0, -200.0), up, 0, 1.0), rw.Node((300.0, 0.0, 0.0), None, None, 1.0)]
    assert rw.balance_weight(back, 2, 8)[:2] == (1.0 / 3.0, "ratio")
    assert rw.balance_weight(back, 0, 8)[0] + rw.balance_weight(back, 1, 8)[0] == pytest.approx(1.0)


def compare_mode_frame(oracle_mod, osc, mode, fr, depth, roulette, seed, num_pairs):
    """pair by pair the oracle's compute_energy(pair_begin = i, pair_end = i + 1) against the model's contributions -> the largest
    relative difference of a (band, bin) entry.  Every pair: step and connection counters.  Every pair without a flagged contribution:
    the deposit count, the occupied bins, every (band, bin) energy to the mode's tolerance."""
    flags, rtol = MODES[mode]
    p = oracle_mod.default_params(num_pairs=num_pairs, depth=depth, seed=seed, russian_roulette=int(roulette), flags=flags)
    prefix = isinstance(fr, rw.PrefixFrame)
    worst, steps, connections, compared = 0.0, 0, 0, 0
    for i, r in enumerate(fr.pairs):
        e32, e64, cnt = osc.compute_energy(p, rw.SOURCE, rw.LISTENER, pair_begin=i, pair_end=i + 1)
        steps += cnt.closest_rays
        connections += cnt.any_rays
        assert cnt.closest_rays == r.steps and cnt.path_nodes == len(r.fwd) + len(r.bwd), (seed, i)
        assert cnt.any_rays == (r.connections if prefix else 1), (seed, i)
        H = np.zeros((4, 1000))
        if prefix:
            if r.flagged:
                continue
            deposits = 0
            for c in r.contributions:
                if c.visible:
                    deposits += 1
                    H[:, c.bin] += c.energy
        else:
            if r.fragile:
                continue
            deposits = int(r.visible)
            if r.visible:
                H[:, r.bin] += r.energy
        compared += 1
        assert cnt.deposits == deposits, (seed, i)
        assert np.array_equal(e64 != 0.0, H != 0.0), (seed, i)
        nz = H != 0.0
        if nz.any():
            d = float(np.abs(e64[nz] / H[nz] - 1.0).max())
            worst = max(worst, d)
            assert d <= rtol, (seed, i, d)
    assert steps == fr.steps and connections == fr.connections
    return worst, compared


FRAMES = [(2, True, 1024), (4, True, 1024), (8, True, 1024), (8, False, 256)]


@pytest.mark.parametrize("depth,roulette,num_pairs", FRAMES, ids=["d2", "d4", "d8", "d8_norr"])
@pytest.mark.parametrize("mode", list(MODES))
def test_mode_frames_against_the_model(oracle_mod, mode, depth, roulette, num_pairs):
    """The oracle in the three build-owned modes against the model's restatement of DESIGN.md section 8: seeds 101, 202, 303,
    1024 pairs at depth 2, 4, 8 with roulette and 256 pairs at depth 8 without.  Conditions on
    a frame, asserted: at most 2 % of its connections tested are flagged; the balance-heuristic frames fall back on degenerate
    segments (the `ratio` fallback cannot occur under a depth cap: a strategy's own density is a product of densities the walks
    sampled, all positive; test_unbounded_depth_against_the_model has it); every lobe frame picks each lobe 100 times or more; the
    all-prefix frames of depth 8 have pairs of more than 64 prefix combinations.
    Measured (CPU, oracle against model; the constants of MODES are 4 x the largest of a mode, the depth-0 frames included):

      mode           flagged, depth 2 / 4 / 8 / 8 without roulette                 largest relative difference, same order
      uniform        0.01 % / 0.02-0.06 % / 0.06-0.19 % / 0.09-0.34 %              4.9e-6 / 1.1e-5 / 7.6e-5 / 4.6e-5
      balance        0.01 % / 0.02-0.06 % / 0.06-0.20 % / 0.09-0.38 %              4.9e-5 / 7.7e-5 / 1.7e-4 / 5.1e-5
      lobes          0-0.39 % / 0.10-0.39 % / 0.10-0.29 % / 0.39-1.56 %            2.0e-6 / 6.0e-6 / 3.7e-5 / 3.1e-4
      lobes_all      0-0.15 % / 0.09-0.18 % / 0.24-0.28 % / 0.24-0.43 %            2.0e-6 / 5.8e-6 / 3.0e-5 / 1.7e-5
      lobes_cosine   0-0.39 % / 0.10-0.39 % / 0.20-0.78 % / 0-1.56 %               1.3e-6 / 2.8e-6 / 5.9e-5 / 1.2e-5

    No pair without a flagged contribution disagreed in any frame.  The balance heuristic's differences are those of grazing
    cosines (a factor of the weight whose relative float32 error is large); they stay within a few 1e-4, so no floor on the cosine is
    used beyond rw.COSINE_FLOOR.  The lobe mode's 3.1e-4 is one pair of seed 101 without roulette: drift through a chain of specular
    bounces, where no cone sample renews the direction.  81 prefix combinations at most: 214 ... 256 pairs of a depth-8 frame have
    more than 64."""
    sc, osc = mode_scene(oracle_mod, mode)
    flags = MODES[mode][0]
    for seed in (101, 202, 303):
        fr = mode_frame(mode, depth, roulette, seed, num_pairs, keep_pairs=True)
        nfr = flagged_contributions(fr)
        worst, compared = compare_mode_frame(oracle_mod, osc, mode, fr, depth, roulette, seed, num_pairs)
        print(f"{mode} depth {depth} roulette {roulette} seed {seed}: flagged {nfr} of {fr.connections} ({nfr / fr.connections:.2%}) pairs compared "
              f"{compared} deposits {fr.deposits} lobes {fr.lobes} worst energy {worst:.3e}"
              + (f" fallbacks {fr.fallbacks} pairs over 64 combinations {fr.pairs_over_64}" if isinstance(fr, rw.PrefixFrame) else ""))
        assert nfr <= 0.02 * fr.connections
        assert compared >= 0.8 * num_pairs and fr.deposits > num_pairs // 10
        if flags & LOBES:
            assert min(fr.lobes) >= 100
        if flags & MIS:
            assert fr.fallbacks["segment"] > 0
        if flags & (ALLC | MIS) and depth == 8:
            assert fr.pairs_over_64 > 0 and 64 < fr.most_combinations <= 81


UNBOUNDED_SEED = 128


@pytest.mark.parametrize("mode", ["uniform", "balance"])
def test_unbounded_depth_against_the_model(oracle_mod, mode):
    """depth 0 (while (true): D is infinite, N(t) = t + 1, every strategy counts), 256 pairs, the two all-prefix modes.  Seed 128:
    the first from 101 on whose frame meets both conditions, at most 2 % of the connections flagged and both fallbacks of the
    weight (of the seeds 101 ... 220 six meet the first: a frame's connections are mostly those of its longest walks, and from
    turn 25 ... 45 on even the per-axis bound calls a walk's decisions fragile, as the float32 walk's drift of up to 1 cm there
    warrants; seed 101 has 9 % flagged, a walk of 84 nodes among them).  The `ratio` fallback occurs only here, where the product
    of more than 40 densities underflows; the model flags those contributions.
    Measured: 407 (uniform) and 411 (balance) of 22 623 connections flagged (1.8 %), 228 pairs compared, largest relative difference
    4.7e-5 in both modes; 9 489 `segment` and 13 `ratio` fallbacks; 660 prefix combinations in one pair."""
    sc, osc = mode_scene(oracle_mod, mode)
    fr = mode_frame(mode, 0, True, UNBOUNDED_SEED, 256, keep_pairs=True)
    worst, compared = compare_mode_frame(oracle_mod, osc, mode, fr, 0, True, UNBOUNDED_SEED, 256)
    print(f"{mode} depth 0: flagged {fr.flagged} of {fr.connections} ({fr.flagged / fr.connections:.2%}) pairs compared {compared} "
          f"worst energy {worst:.3e} fallbacks {fr.fallbacks} most combinations {fr.most_combinations}")
    assert compared > 128 and fr.most_combinations > 81
    if mode == "balance":
        assert fr.fallbacks["segment"] > 0 and fr.fallbacks["ratio"] > 0
    assert fr.flagged <= 0.02 * fr.connections
