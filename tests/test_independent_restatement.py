"""An INDEPENDENT float64 restatement of the path — written from the reference's lines, not from oracle/fs_oracle.c —
checked against the C oracle on thousands of random inputs.  The closed-form pieces:

  EvaluatePath                 Private/AudioRayTracingSubsystem.cpp:358-420
  AddEnergyAtDelay (bin rule)  Public/FrequenSeeAudioComponent.h:87-91
  ReconstructImpulseResponse   Private/FrequenSeeAudioComponent.cpp:320-380 (+ NormalizeImpulseResponse :382-406)

and, with the model of tests/restate_walk.py (axis-aligned rectangles intersected analytically, every discrete decision
with a margin), the walk and the connection:

  GeneratePath                 Private/AudioRayTracingSubsystem.cpp:279-355   step by step on uncapped walks
  ConnectSubpaths              Private/AudioRayTracingSubsystem.cpp:235-277   verdicts; node order through whole pairs

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
