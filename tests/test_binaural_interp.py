"""fs_binaural_render_process_batch with a mesh on the HRIR set (fs_hrtf_set_mesh): every voice's per-ear HRIR is the barycentric
blend of the three at the corners of the spherical triangle its direction falls in (include/frequensee.h, rules 2', 3' and 6').

The yardstick is MeshModel: the nearest-mode Model of test_binaural_render.py with the HRIR index replaced by (t, b[3]) from the
numpy float32 restatement of fs_hrtf_mesh_locate and the HRIR by the fp32 blend — which the device must EQUAL (tobytes()).  Beside
it the same rule in float64 under a derived bound, known answers that need no restatement, nearest mode itself where the two must
agree, and the state, batch and plumbing rules."""
import ctypes as C

import numpy as np
import pytest

import test_binaural_render as nearest_mode
from hrtf_mesh_model import OCTAHEDRON, SETS, fibonacci, locate32, rows64
from test_binaural_render import Model, assert_same, bound64, entry, one
from test_direct_paths import device_free_bytes
from test_direct_render import F32, FS
from test_direct_render import _close_contexts  # noqa: F401  (closes the contexts ctx_for caches when this module is done)
from test_direct_render import ctx_for, mix_model, noise, table_of
from test_reflection_paths import LIS, SRC, shoebox_world
from test_reflection_render import POW2_FS, bank_schedule

U = 2.0 ** -24


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
class Blend(np.ndarray):
    """an fp32 HRIR blended by rule 3'; as float64 it is the exact blend with the float64 weights — what Model.process builds its
    float64 side from (h.astype(np.float64))"""

    def astype(self, dtype, *args, **kwargs):
        if np.dtype(dtype) == np.float64:
            return self.exact
        return np.asarray(self).astype(dtype, *args, **kwargs)


class BlendedSet:
    """hrir[(t, b, b64, werr), ear]: hA[k] = (bA_0 * h[v_0][ear][k] + bA_1 * h[v_1][ear][k]) + bA_2 * h[v_2][ear][k], fp32"""

    def __init__(self, hrir, tri):
        self.h, self.tri, self.shape = np.asarray(hrir, np.float32), np.asarray(tri), np.shape(hrir)

    def __getitem__(self, key):
        (t, b, b64, _), ear = key
        h = [self.h[v, ear] for v in self.tri[t]]
        out = ((b[0] * h[0] + b[1] * h[1]) + b[2] * h[2])
        assert out.dtype == np.float32
        out = out.view(Blend)
        out.exact = sum(b64[i] * h[i].astype(np.float64) for i in range(3))
        return out


class MeshModel(Model):
    """Model with a mesh in force: what a slot holds and an entry aims at is (t, b[3]) from fs_hrtf_mesh_locate's restatement —
    carried as (t, b, the float64 weights, the bound on the blend's error per corner: weight_error) — and the HRIR their blend.
    The matching, the fold and the tap loop are Model's own: its `nearest` is this model's locate while it matches."""

    def __init__(self, table, dirs, hrir, tri, rows, frame, voices, fs=FS):
        super().__init__(table, dirs, hrir, frame, voices, fs)
        self.set_mesh(tri, rows)

    def set_mesh(self, tri, rows):
        """fs_hrtf_set_mesh: every held slot is free, the history stays"""
        self.tri, self.rows = np.asarray(tri), np.asarray(rows, np.float32)
        self.rows64 = rows64(self.dirs, self.tri)[0]
        self.hrir = BlendedSet(self.hrir.h if isinstance(self.hrir, BlendedSet) else self.hrir, self.tri)
        self.slots = [None] * self.V

    def locate(self, d):
        d = np.asarray(d, np.float32)
        t, b = locate32(self.rows, d)
        # the same triangle in float64: g* = r* . d, c* = max(g*, 0), b* = c* / s*
        terms = self.rows64[t] * d.astype(np.float64)[None, :]
        c = np.maximum(terms.sum(1), 0.0)
        s = c.sum()
        return t, b, c / s, weight_error(np.abs(terms).sum(1), c, s)

    def match(self, entries):
        keep = nearest_mode.nearest
        nearest_mode.nearest = lambda dirs, d: self.locate(d)
        try:
            return super().match(entries)
        finally:
            nearest_mode.nearest = keep


def weight_error(G, c, s):
    """|hA[k] - sum_i b*_i h_i[k]| <= sum_i weight_error_i |h_i[k]|, derived, with u = 2^-24, G_i = sum_c |d_c r*_ic|:
    a row component is rounded once, its product with d_c once, and the dot product's two sums round again: |g_i - g*_i| <=
    ((1 + u)^4 - 1) G_i = eps_i, and clamping at 0 does not widen it.  s = (c_0 + c_1) + c_2 of non-negative terms: |s - s*| <=
    sum eps + ((1 + u)^2 - 1) (s* + sum eps) = E.  b_i = fl(c_i / s): |b_i - b*_i| <= (eps_i + b*_i E) / (s* - E) (1 + u) + u b*_i
    = delta_i.  The blend multiplies (one rounding) and sums twice: a term sees at most three roundings, so its error is at most
    delta_i (1 + u)^3 |h_i| + ((1 + u)^3 - 1) b*_i |h_i|."""
    eps = ((1.0 + U) ** 4 - 1.0) * G
    E = eps.sum() + ((1.0 + U) ** 2 - 1.0) * (s + eps.sum())
    b = c / s
    delta = (eps + b * E) / (s - E) * (1.0 + U) + U * b
    return delta * (1.0 + U) ** 3 + ((1.0 + U) ** 3 - 1.0) * b


def blend_bound(m, entries, peak=1.0):
    """What the blend adds to bound64 when the float64 side blends exactly, for the callback m.process(entries) is about to run:
    the folded table is linear in the HRIR, so an HRIR off by dh[k] moves sum_u |C[u]| by at most (sum_k |dh[k]|) (sum_t |f[t]|),
    and the output by max|x| times that times the voice's weight — summed over the voices, the larger of the two ends and ears, as
    bound64's weights are."""
    plan, _ = m.match(entries)
    k64 = np.abs(m.k.astype(np.float64))
    total = 0.0
    for p in plan:
        if p is None:
            continue
        kind, d0, g0, w0, q0, d1, g1, w1, q1, key = p
        worst = 0.0
        for q, g in ((q0, g0), (q1, g1)):
            f_sum = (np.abs(g.astype(np.float64)) @ k64).sum()
            for ear in range(2):
                dh = sum(q[3][i] * np.abs(m.hrir.h[v, ear].astype(np.float64)).sum() for i, v in enumerate(m.tri[q[0]]))
                worst = max(worst, dh * f_sum)
        total += float(max(abs(w0), abs(w1))) * worst
    return peak * total


def mesh_set(pkg, n, H, rng):
    """(dirs, hrir, tri, rows): a set of n directions with random HRIRs of H taps, triangulated by the library, its triangles
    shuffled and each rotated at random, rows by the library's own fs_hrtf_mesh_rows"""
    dirs = {4: SETS["fib4"], 6: OCTAHEDRON, 258: SETS["fib258"], 4096: SETS["fib4096"], 2522: SETS["latlong"]}[n]
    tri = pkg.Context.hrtf_triangulate(dirs)
    tri = np.stack([np.roll(t, int(rng.integers(0, 3))) for t in tri[rng.permutation(tri.shape[0])]]).astype(np.int32)
    return dirs, rng.uniform(-1.0, 1.0, (n, 2, H)).astype(np.float32), tri, pkg.Context.hrtf_mesh_rows(dirs, tri)


def install(ctx, the_set):
    dirs, hrir, tri, rows = the_set
    ctx.hrtf_set(dirs, hrir)
    assert ctx.hrtf_mesh_info() == 0
    ctx.hrtf_set_mesh(tri)
    assert ctx.hrtf_mesh_info() == tri.shape[0] == 2 * dirs.shape[0] - 4


def mesh_schedule(rng, dirs):
    """the reflection renderer's eight-callback script on three slots (bank_schedule) with the first channel gain as the gain and
    a direction per entry that moves in every callback: random ones of any length, set directions (where the triangles round
    them tie or nearly tie), and midpoints of two set directions (an edge, or a chord through a neighbour)"""
    script = []
    for cb, (entries, counts) in enumerate(bank_schedule(rng)):
        lst = []
        for e, (key, delay, gains, chan) in enumerate(entries):
            kind = (cb + e) % 3
            if kind == 0:
                d = rng.normal(size=3) * 10.0 ** rng.uniform(-2, 2)
            elif kind == 1:
                d = dirs[int(rng.integers(0, dirs.shape[0]))] * F32(rng.choice([0.5, 1.0, 7.0]))
            else:
                a, b = rng.integers(0, dirs.shape[0], 2)
                d = dirs[a] + dirs[b] if a != b and not np.allclose(dirs[a], -dirs[b]) else dirs[a]
            lst.append((key, delay, gains, float(chan[0]), np.asarray(d, np.float32)))
        script.append((lst, counts))
    return script


def test_exports(pkg):
    lib = pkg._capi.load()
    for name in ("fs_hrtf_triangulate", "fs_hrtf_mesh_rows", "fs_hrtf_mesh_locate", "fs_hrtf_set_mesh", "fs_hrtf_mesh_info"):
        assert name in pkg._capi.EXPORTS and hasattr(lib, name)
    assert lib.fs_abi_version() == 5


def test_restatement_against_float64(pkg):
    """The float32 restatement lies inside bound64 — test_binaural_render's, derived there — plus blend_bound, derived above: the
    float64 side takes the triangle from the fp32 rule and computes the weights, the blend, the fold and the tap loop in float64.
    40 random cases, K <= 3 voices, the second callback ramping delays, gains and directions; the worst observed share of the
    bound is printed (DESIGN.md records it).  (bound64's W_fold is formed with the exact blend's magnitudes in the place of the
    fp32 blend's: they differ by the blend's error, a factor of 1 + O(2^-24) on a term that carries 2^-24 already.)"""
    rng = np.random.default_rng(0xB1A1)
    worst = blend_share = 0.0
    for case in range(40):
        bands, taps, H, frame = int(rng.choice([1, 3, 8])), int(rng.choice([15, 63])), int(rng.choice([2, 7, 32])), 32
        K = int(rng.integers(1, 4))
        dirs, hrir, tri, rows = mesh_set(pkg, (6, 258, 4)[case % 3], H, rng)
        m = MeshModel(pkg.Context.direct_band_kernels(FS, bands, taps), dirs, hrir, tri, rows, frame, K)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            entries = [(k, float(rng.uniform(0.0, 300.0)) / FS, rng.uniform(0.0, 1.0, 8), float(rng.uniform(-1.0, 1.0)),
                        dirs[int(rng.integers(0, dirs.shape[0]))] if (case + k) % 4 == 0 else rng.normal(size=3)) for k in range(K)]
            extra = blend_bound(m, entries)
            y, row, y64, w_loop, w_fold = m.process(blk, entries, want64=True)
        assert row == (K, 0, 0, 0)
        bound = bound64(taps, H, bands, K, w_loop, w_fold) + extra
        worst = max(worst, float(np.abs(y - y64).max() / bound))
        blend_share = max(blend_share, extra / bound)
    print(f"restatement vs float64 with a mesh: worst share of the bound {worst:.3f} (the blend's term is at most {blend_share:.3f} of it)")
    assert worst <= 1.0


# ---- GPU -------------------------------------------------------------------------------------------------------------------
# every B, F, T, H and n the rule names at least once, the large ones together and apart: (bands, frame, taps, H, n); the last has
# m = 8188 triangles: 127 full strides of 64 and a ragged one of 60
SHAPES = [(1, 64, 1, 1, 4), (3, 64, 15, 7, 6), (8, 64, 255, 128, 258), (8, 320, 15, 128, 4), (3, 320, 255, 7, 6), (1, 320, 1, 7, 258),
          (3, 64, 1, 128, 6), (8, 320, 255, 1, 258), (1, 64, 15, 7, 4), (3, 64, 1, 2, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("bands,frame,taps,H,n", SHAPES)
def test_bit_equal_to_the_restatement(pkg, bands, frame, taps, H, n):
    ctx = ctx_for(pkg, bands)
    rng = np.random.default_rng(2000 * bands + frame + taps + 7 * H + n)
    the_set = mesh_set(pkg, n, H, rng)
    install(ctx, the_set)
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, taps, 3, 0.02)
    m = MeshModel(table_of(pkg, ctx, taps), *the_set, frame, 3)
    for cb, (entries, counts) in enumerate(mesh_schedule(rng, the_set[0])):
        blk = noise(rng, 1, frame)[0]
        want = m.process(blk, entries)
        assert want[1] == counts, f"callback {cb + 1}: the yardstick's own counts"
        assert_same(one(ctx, src, blk, entries), want, f"callback {cb + 1}")
    ctx.destroy_source(src)
    ctx.hrtf_set_mesh(None)


@pytest.mark.gpu
def test_ties_on_the_device(pkg):
    """the 72 x 35 lat-long set with exact poles and an exact (1, 0, 0), its 5040 triangles shuffled: a voice at a pole has mu = 0
    in all 72 triangles round it — in many lanes and strides of the device's search — and must come out in the restatement's, the
    lowest; there its weights are exactly (1, 0, 0) up to the corner's place, so the output equals nearest mode's on the same set
    by value"""
    rng = np.random.default_rng(72)
    frame, taps, H = 64, 15, 7
    the_set = mesh_set(pkg, 2522, H, rng)
    dirs, hrir, tri, rows = the_set
    queries = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 2.5), (0.0, 0.0, -0.125), (3.0, 0.0, 0.0)]
    for d in queries[:3]:
        t, b = locate32(rows, d)
        g = (F32(d[0]) * rows[:, :, 0] + F32(d[1]) * rows[:, :, 1]) + F32(d[2]) * rows[:, :, 2]
        tied = np.nonzero(g.min(1) == g.min(1).max())[0]
        assert tied.size >= (72 if d[2] else 4) and t == tied.min(), (d, tied)
        if d[2]:   # many lanes, and more than one triangle in some lane: ties within a lane's stride and across lanes
            lanes = [int(j) % 64 for j in tied]
            assert len(set(lanes)) > 16 and len(set(lanes)) < len(lanes), (d, tied)
        assert sorted(b.tolist()) == [0.0, 0.0, 1.0]
    ctx, plain = ctx_for(pkg, 3), pkg.Context(num_bands=3)
    install(ctx, the_set)
    plain.hrtf_set(dirs, hrir)
    a, b = ctx.create_source(), plain.create_source()
    ctx.binaural_render_init(a, frame, taps, len(queries), 0.02)
    plain.binaural_render_init(b, frame, taps, len(queries), 0.02)
    m = MeshModel(table_of(pkg, ctx, taps), *the_set, frame, len(queries))
    g = rng.uniform(0, 1, 8).astype(np.float32)
    entries = [entry(k, 30.5 + k, g, 0.7, d) for k, d in enumerate(queries)]
    for cb in range(2):
        blk = noise(rng, 1, frame)[0]
        got = one(ctx, a, blk, entries)
        assert_same(got, m.process(blk, entries), f"callback {cb + 1}")
        near = one(plain, b, blk, entries)
        assert got[1] == near[1] and np.array_equal(got[0], near[0]), f"callback {cb + 1}: not nearest mode's output"
    assert got[0].any()
    ctx.destroy_source(a)
    ctx.hrtf_set_mesh(None)
    plain.close()


# ---- behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_centroid_of_delta_hrirs(pkg):
    """the octahedron, HRIRs that are a delta at tap j (left) and tap 6 + j (right) for direction j, one band (its kernel of T = 1
    is exactly 1), unit gains, a held voice at 20 samples from (1, 1, 1) — the centroid of the triangle on +x, +y, +z (directions
    0, 2, 4), whose rows are exact: g = (1, 1, 1), b = 1.0f / 3.0f each.  An impulse comes out as exactly that at 20 + 0, 2, 4
    left and 20 + 6, 8, 10 right, and exactly 0 elsewhere"""
    ctx = ctx_for(pkg, 1, POW2_FS)
    hrir = np.zeros((6, 2, 12), np.float32)
    for j in range(6):
        hrir[j, 0, j] = hrir[j, 1, 6 + j] = 1.0
    tri = pkg.Context.hrtf_triangulate(OCTAHEDRON)
    ctx.hrtf_set(OCTAHEDRON, hrir)
    ctx.hrtf_set_mesh(tri)
    frame = 64
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, 1, 2, 0.001)
    entries = [(1, 20.0 / POW2_FS, np.ones(8, np.float32), 1.0, (1.0, 1.0, 1.0))]
    one(ctx, src, np.zeros(2 * frame, np.float32), entries)   # the voice fades in on silence: held from here on
    blk = np.zeros(2 * frame, np.float32)
    blk[0] = blk[1] = 1.0
    out, row = one(ctx, src, blk, entries)
    assert row == (1, 0, 0, 0)
    third = F32(1.0) / F32(3.0)
    want = np.zeros(2 * frame, np.float32)
    for j in (0, 2, 4):
        want[2 * (20 + j)] = want[2 * (20 + 6 + j) + 1] = third
    assert np.array_equal(out, want)
    ctx.destroy_source(src)
    ctx.hrtf_set_mesh(None)


@pytest.mark.gpu
def test_a_corner_is_nearest_mode_and_voices_fade(pkg):
    """n = 258, random HRIRs.  Source A has the mesh, source N (another context) has not; B has the mesh and holds its voices
    steadily.  Every voice points at a set direction, where the exact weights are (1, 0, 0): A and N are each within their own
    bound of the same exact output.  Then, on the same blocks: A's voices start one callback after B's — that callback is a(s)
    times B's; they end one callback before B's — that one is (1 - a(s)) times B's, on the triangle and weights they held —
    each within the two sources' bounds"""
    rng = np.random.default_rng(258)
    frame, taps, H, K = 64, 15, 7, 3
    the_set = mesh_set(pkg, 258, H, rng)
    dirs, hrir, tri, rows = the_set
    ctx, plain = ctx_for(pkg, 3), pkg.Context(num_bands=3)
    install(ctx, the_set)
    plain.hrtf_set(dirs, hrir)
    a, b, n = ctx.create_source(), ctx.create_source(), plain.create_source()
    for c, s in ((ctx, a), (ctx, b), (plain, n)):
        c.binaural_render_init(s, frame, taps, 4, 0.02)
    table = table_of(pkg, ctx, taps)
    mb, mn = MeshModel(table, *the_set, frame, 4), Model(table, dirs, hrir, frame, 4)
    entries = [entry(k, rng.uniform(0, 300), rng.uniform(0, 1, 8), rng.uniform(0.3, 1.0) * (-1) ** k, dirs[int(rng.integers(0, 258))] * F32(1.5))
               for k in range(K)]
    ramp = np.repeat(((np.arange(frame) + 1).astype(np.float32) / F32(frame)).astype(np.float64), 2)
    for cb, (a_list, scale) in enumerate((([], None), (entries, ramp), (entries, None), ([], 1.0 - ramp))):
        blk = noise(rng, 1, frame)[0]
        extra = blend_bound(mb, entries)
        got_a, got_b, got_n = one(ctx, a, blk, a_list), one(ctx, b, blk, entries), one(plain, n, blk, entries)
        want_b, want_n = mb.process(blk, entries, want64=True), mn.process(blk, entries, want64=True)
        assert_same(got_b, want_b[:2], f"callback {cb + 1}")
        assert_same(got_n, want_n[:2], f"callback {cb + 1}, nearest mode")
        bound_b = bound64(taps, H, 3, K, want_b[3], want_b[4]) + extra
        bound_n = bound64(taps, H, 3, K, want_n[3], want_n[4])
        B, N = got_b[0].astype(np.float64), got_n[0].astype(np.float64)
        assert np.all(np.abs(B - N) <= bound_b + bound_n), f"callback {cb + 1}: a corner is not nearest mode"
        assert np.abs(N).max() > 1000 * (bound_b + bound_n)
        if scale is None:
            if cb == 2:
                assert_same(got_a, got_b, "both steady")
            continue
        assert got_a[1] == ((K, K, 0, 0) if cb == 1 else (K, 0, K, 0))
        assert np.all(np.abs(got_a[0].astype(np.float64) - scale * B) <= 2 * bound_b), f"callback {cb + 1}: not B's block times the ramp"
    for s in (a, b):
        ctx.destroy_source(s)
    ctx.hrtf_set_mesh(None)
    plain.close()


@pytest.mark.gpu
def test_alternating_direction_is_a_crossfade(pkg):
    """source A's one voice points into two different triangles in turn; B and C hold it steadily in one and in the other; the
    same input, delay and gains.  The coefficient C0[u] + a dC[u] is linear in the two tables, so in exact arithmetic A =
    (1 - a) y_0 + a y_1 sample by sample; each of the three is within its bound of its exact value, so the comparison is held to
    A's bound plus the larger of the other two.  No voice starts or ends"""
    rng = np.random.default_rng(18)
    frame, taps, H = 320, 15, 7
    the_set = mesh_set(pkg, 258, H, rng)
    ctx = ctx_for(pkg, 3)
    install(ctx, the_set)
    srcs = [ctx.create_source() for _ in range(3)]
    for s in srcs:
        ctx.binaural_render_init(s, frame, taps, 2, 0.02)
    table = table_of(pkg, ctx, taps)
    models = [MeshModel(table, *the_set, frame, 2) for _ in range(3)]
    gains = rng.uniform(0, 1, 8).astype(np.float32)
    aims = [(0.3, 0.9, 0.2), (0.35, 0.8, -0.4)]
    assert models[0].locate(aims[0])[0] != models[0].locate(aims[1])[0]
    a = np.repeat(((np.arange(frame) + 1).astype(np.float32) / F32(frame)).astype(np.float64), 2)
    worst = 0.0
    for cb in range(5):
        blk = noise(rng, 1, frame)[0]
        q0, q1 = (cb + 1) % 2, cb % 2   # what A comes from and goes to
        lists = [[entry(1, 200.4, gains, 1.0, aims[q1])], [entry(1, 200.4, gains, 1.0, aims[0])], [entry(1, 200.4, gains, 1.0, aims[1])]]
        extras = [blend_bound(m, lst) for m, lst in zip(models, lists)]
        out, rows = ctx.binaural_render_process_batch(srcs, np.stack([blk] * 3), lists)
        wants = [m.process(blk, lst, want64=True) for m, lst in zip(models, lists)]
        for i in range(3):
            assert_same((out[i], tuple(int(x) for x in rows[i])), wants[i][:2], f"callback {cb + 1}, source {i}")
        if cb == 0:
            continue   # all three fade in
        bounds = [bound64(taps, H, 3, 1, w[3], w[4]) + x for w, x in zip(wants, extras)]
        steady = [out[1].astype(np.float64), out[2].astype(np.float64)]
        diff = np.abs(out[0].astype(np.float64) - ((1.0 - a) * steady[q0] + a * steady[q1]))
        bound = bounds[0] + max(bounds[1:])
        worst = max(worst, float(diff.max() / bound))
        assert np.all(diff <= bound), f"callback {cb + 1}"
        assert np.abs(steady[0] - steady[1]).max() > 100 * bound, "the two directions sound different"
    print(f"alternating direction with a mesh: worst share of the bound {worst:.3f}")
    for s in srcs:
        ctx.destroy_source(s)
    ctx.hrtf_set_mesh(None)


# ---- state and plumbing ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mesh_changes_start_every_voice_and_refusals_change_nothing(pkg):
    """voices held in nearest mode; fs_hrtf_set_mesh: the next callback reports them all as started, and is the mesh model's from
    free slots on the kept history; a refused mesh in between changes nothing — the voices go on, bit for bit; clearing the mesh
    starts them again, in nearest mode, and from there on the outputs are those of a context that never had a mesh; fs_hrtf_set
    drops the mesh"""
    cap = pkg._capi
    rng = np.random.default_rng(19)
    frame, taps, H, K = 64, 15, 7, 3
    the_set = mesh_set(pkg, 258, H, rng)
    dirs, hrir, tri, rows = the_set
    ctx, never = pkg.Context(num_bands=3), pkg.Context(num_bands=3)
    lib = ctx.lib
    assert lib.fs_hrtf_set_mesh(ctx.h, tri.ctypes.data, tri.shape[0]) == cap.ERR_INVALID_ARGUMENT, "no set in force"
    assert lib.fs_hrtf_mesh_info(None, None) == cap.ERR_INVALID_ARGUMENT and lib.fs_hrtf_set_mesh(None, None, 0) == cap.ERR_INVALID_ARGUMENT
    for c in (ctx, never):
        c.hrtf_set(dirs, hrir)
    a, b = ctx.create_source(), never.create_source()
    ctx.binaural_render_init(a, frame, taps, 4, 0.02)
    never.binaural_render_init(b, frame, taps, 4, 0.02)
    table = table_of(pkg, ctx, taps)
    near, mesh, other = Model(table, dirs, hrir, frame, 4), MeshModel(table, *the_set, frame, 4), Model(table, dirs, hrir, frame, 4)

    def callback(model, started):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(k, rng.uniform(0, 300), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(K)]
        for m in (near, mesh):   # both models hear every block: the history is kept across the modes
            want = m.process(blk, entries)
            if m is model:
                got = one(ctx, a, blk, entries)
                assert_same(got, want, "the mode's own model")
        assert got[1] == (K, K if started else 0, 0, 0)
        return got, one(never, b, blk, entries), other.process(blk, entries)

    callback(near, True)
    callback(near, False)
    flipped = tri.copy()
    flipped[11] = flipped[11][::-1]
    refused = [(flipped, tri.shape[0]), (tri, tri.shape[0] - 1), (tri, -1)]
    for t, m in refused:
        assert lib.fs_hrtf_set_mesh(ctx.h, t.ctypes.data, m) == cap.ERR_INVALID_ARGUMENT
    assert ctx.hrtf_mesh_info() == 0
    callback(near, False)   # nothing started anew
    ctx.hrtf_set_mesh(tri)
    mesh.slots = [None] * 4
    assert ctx.hrtf_mesh_info() == tri.shape[0]
    callback(mesh, True)
    callback(mesh, False)
    for t, m in refused:
        assert lib.fs_hrtf_set_mesh(ctx.h, t.ctypes.data, m) == cap.ERR_INVALID_ARGUMENT
    assert ctx.hrtf_mesh_info() == tri.shape[0]
    callback(mesh, False)   # the mesh and the held voices are as they were
    ctx.hrtf_set_mesh(None)
    near.slots = [None] * 4
    assert ctx.hrtf_mesh_info() == 0
    never.hrtf_set(dirs, hrir)   # (the other context's voices start at the same callback)
    other.set(dirs, hrir)
    for cb in range(2):
        got, plain, want = callback(near, cb == 0)
        assert_same(plain, want, "the context that never had a mesh")
        assert_same(got, plain, "after clearing the mesh: not a context's that never had one")
    ctx.hrtf_set_mesh(tri)
    ctx.hrtf_set(dirs, hrir)   # a set, new or not, drops the mesh
    assert ctx.hrtf_mesh_info() == 0 and ctx.hrtf_info() == (258, H)
    near.slots = [None] * 4
    callback(near, True)
    ctx.hrtf_set_mesh(tri)
    ctx.hrtf_set(None, None)
    assert ctx.hrtf_mesh_info() == 0
    ctx.close()
    never.close()


@pytest.mark.gpu
def test_batch_single_and_permuted_agree(pkg):
    """sources of 1, 3 and 8 slots with 0, 1 and 5 entries (rotating) in one batch of stride 5, with a mesh"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(4)
    frame, taps, n = 320, 15, 3
    the_set = mesh_set(pkg, 258, 7, rng)
    install(ctx, the_set)
    V = [1, 3, 8]
    sets = [[ctx.create_source() for _ in range(n)] for _ in range(3)]   # one call | three calls | permuted order
    for group in sets:
        for s, v in zip(group, V):
            ctx.binaural_render_init(s, frame, taps, v, 0.02)
    models = [MeshModel(table_of(pkg, ctx, taps), *the_set, frame, v) for v in V]
    perm = [2, 0, 1]
    counts = [[0, 1, 5], [1, 5, 0], [5, 0, 1], [1, 1, 5]]
    for cb in range(4):
        blk = noise(rng, n, frame)
        lists = [[entry(50 + k, rng.uniform(0, 600), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(counts[cb][i])]
                 for i in range(n)]
        out, mix, rows = ctx.binaural_render_process_batch(sets[0], blk, lists, stride=5, want_mix=True)
        singles = [one(ctx, sets[1][i], blk[i], lists[i], stride=5) for i in range(n)]
        pout, pmix, prows = ctx.binaural_render_process_batch([sets[2][i] for i in perm], blk[perm], [lists[i] for i in perm], stride=5,
                                                              want_mix=True)
        for i in range(n):
            want = models[i].process(blk[i], lists[i])
            assert_same((out[i], tuple(int(x) for x in rows[i])), want, f"batch {cb} {i}")
            assert_same(singles[i], want, f"single {cb} {i}")
            j = perm.index(i)
            assert_same((pout[j], tuple(int(x) for x in prows[j])), want, f"permuted {cb} {i}")
        assert mix.tobytes() == mix_model(out).tobytes(), "mix is not the fp32 sum in list order"
        assert pmix.tobytes() == mix_model(pout).tobytes()
    for s in sum(sets, []):
        ctx.destroy_source(s)
    ctx.hrtf_set_mesh(None)


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    ctx = pkg.Context(num_bands=3)
    rng = np.random.default_rng(41)
    install(ctx, mesh_set(pkg, 258, 32, rng))
    frame, taps, n = 64, 15, 40
    srcs = [ctx.create_source() for _ in range(n)]
    for s in srcs:
        ctx.binaural_render_init(s, frame, taps, 4, 0.01)
    blk = noise(rng, n, frame)
    lists = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.0)) for k in range(3)]] * n
    ctx.binaural_render_process_batch(srcs, blk, lists[:n], stride=4, want_mix=True)
    free0 = device_free_bytes()
    for cb in range(20):
        more = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.1 * cb)) for k in range(cb % 2, 4)]] * n   # slots fill up and turn over
        ctx.binaural_render_process_batch(srcs, blk, more, stride=4, want_mix=True)
    ctx.binaural_render_process_batch(srcs[:7], blk[:7], lists[:7], stride=3)   # a smaller shape fits what is there
    assert device_free_bytes() >= free0
    ctx.close()


@pytest.mark.gpu
def test_release_and_reinit(pkg):
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(9)
    the_set = mesh_set(pkg, 6, 7, rng)
    install(ctx, the_set)
    src = ctx.create_source()
    frame, taps, V = 64, 15, 3
    ctx.binaural_render_init(src, frame, taps, V, 0.02)
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    entries = [entry(1, 50.5, g[0], 1.0, (0.0, 1.0, 0.2)), entry(2, 300.0, g[1], -0.5, (1.0, -1.0, 0.0))]
    for _ in range(2):
        one(ctx, src, noise(rng, 1, frame)[0], entries)
    ctx.binaural_render_release(src)   # zero history, every slot free: the same keys fade in from silence
    m = MeshModel(table_of(pkg, ctx, taps), *the_set, frame, V)
    for cb in range(2):
        blk = noise(rng, 1, frame)[0]
        got = one(ctx, src, blk, entries)
        assert got[1] == (2, 2 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"after release, callback {cb + 1}")
    for frame, taps, V in ((320, 15, 1), (64, 63, 5)):   # another F, another T, another V — with voices held
        ctx.binaural_render_init(src, frame, taps, V, 0.02)
        m = MeshModel(table_of(pkg, ctx, taps), *the_set, frame, V)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"{(frame, taps, V)} callback {cb + 1}")
    ctx.destroy_source(src)   # with voices held
    other = ctx.create_source()
    ctx.binaural_render_init(other, 64, 15, 2, 0.02)
    m = MeshModel(table_of(pkg, ctx, 15), *the_set, 64, 2)
    blk = noise(rng, 1, 64)[0]
    assert_same(one(ctx, other, blk, entries), m.process(blk, entries), "a new source after the destroy")
    ctx.destroy_source(other)
    ctx.hrtf_set_mesh(None)
    closing = pkg.Context(num_bands=1)   # fs_context_destroy with a set, a mesh, a source and held voices
    install(closing, the_set)
    s = closing.create_source()
    closing.binaural_render_init(s, 64, 15, 2, 0.02)
    one(closing, s, blk, entries)
    closing.close()


@pytest.mark.gpu
def test_component_layer(pkg):
    """FrequenSeeAudioBinauralPlugin.SetHrtf(interpolate=True) in the 12-triangle shoebox, the listener facing +x, the source
    walking past 100 cm to its right in 48 steps while it plays a sine of a whole number of periods per block: on the same
    64-direction spherical-head set the largest block-to-block change of the per-ear output envelope (the block's RMS) is smaller
    than with interpolate=False — the nearest direction hops between blocks, the blend moves with the source"""
    w = shoebox_world()
    frame, taps = 256, 15
    fwd, right = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    lis = np.asarray(LIS, np.float64)
    sine = np.sin(2.0 * np.pi * 8.0 * np.arange(frame) / frame).astype(np.float32)   # 8 periods a block: every block is the same
    mono = np.repeat(sine, 2)[None]

    def walk(interpolate):
        sub = pkg.AudioRayTracingSubsystem(num_bands=4)
        sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
        sub.SetMaterials(w.absorption, w.transmission, w.scattering)
        comp = pkg.FrequenSeeAudioComponent(SRC)
        comp.OnRegister(sub)
        sub.SetListenerLocation(LIS)
        plug = pkg.FrequenSeeAudioBinauralPlugin(sub)
        plug.Initialize(frame, taps, 16, 0.05)
        plug.SetHrtf(directions=64, taps=64, interpolate=interpolate)
        assert sub.ctx.hrtf_mesh_info() == (124 if interpolate else 0)
        plug.OnInitSource(comp)
        envelope = []
        for dx in np.linspace(-120.0, 120.0, 48):
            comp.SetComponentLocation([float(lis[0] + dx), float(lis[1] + 100.0), float(lis[2])])
            direct = sub.UpdateDirectPaths()
            rows, paths = sub.UpdateReflectionPaths(max_paths=8)
            out, grow = plug.ProcessAudio([comp], mono, rows, paths, fwd, right, reference_length=500.0, direct=(direct, LIS))
            assert int(grow[0]["dropped"]) == 0
            envelope.append([float(np.sqrt(np.mean(out[0][ch::2].astype(np.float64) ** 2))) for ch in range(2)])
        plug.OnReleaseSource(comp)
        sub.Deinitialize()
        return np.abs(np.diff(np.asarray(envelope)[2:], axis=0)).max(axis=0)   # (the first blocks fade in and fill the filter)

    hops, blended = walk(False), walk(True)
    print(f"largest block-to-block change of the envelope, left / right: nearest {hops[0]:.4f} / {hops[1]:.4f}, interpolated {blended[0]:.4f} / {blended[1]:.4f}")
    assert np.all(blended < hops)
