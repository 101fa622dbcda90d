"""fs_update_direct_paths: distance, arrival time, visibility and per-band transmission of every source's direct sound.

The yardstick is a Python restatement of include/frequensee.h's `chain` and per-source rule on numpy float32 scalars (every
operation rounded on its own, fmaf exact).  Each closest hit comes from oracle.Scene.trace_closest(brute=True), the scan
tests/test_gpu_parity.py holds the GPU line trace to bit for bit; the gains from Scene.lobe_table(m)[0][2]; the pass-through rule
from the test's own object ids; the offsets from fs_direct_sample_offsets.  Every field of every row must EQUAL it.
The yardstick itself is checked without a GPU against a float64 brute force (Moeller-Trumbore in double over all triangles,
crossings sorted by t) on the samples whose float64 crossings are not marginal.
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

pytest.register_assert_rewrite("path_query_contract")
import path_query_contract as contract  # noqa: E402
from path_query_contract import device_free_bytes, place  # noqa: E402,F401  (other test files import device_free_bytes from here)

F = np.float32
NO_OBJECT = 0xFFFFFFFF
MAX_QUERIES = 32
DEFAULTS = dict(samples=16, source_radius=0.0, max_surfaces=8, step=0.1, pullback=0.1, dist_divisor=1000.0, sound_speed=343.0)


# ---- exact fp32 pieces ---------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in double; the sum is rounded to odd in double
    (53 >= 2 * 24 + 2 bits), so that the final rounding to float32 is the single rounding of the exact value"""
    p, c = float(a) * float(b), float(c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0 and math.isfinite(s) and (struct.unpack("<q", struct.pack("<d", s))[0] & 1) == 0:
        s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return F(s)


def test_fmaf_helper_rounds_once():
    # 1 + 2^-24 + 2^-60: a sum rounded to double first (1 + 2^-24, a float32 tie) would round to even, 1.0
    assert fmaf(F(2.0 ** -30), F(2.0 ** -30), F(1.0)) == F(1.0)
    a, b, c = F(1.0 + 2.0 ** -12), F(1.0 + 2.0 ** -12), F(2.0 ** -60)   # a b = 1 + 2^-11 + 2^-24: a tie that c breaks upwards
    assert fmaf(a, b, c) == F(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert F(float(a) * float(b) + float(c)) == F(1.0 + 2.0 ** -11)     # ... which plain double arithmetic misses
    assert fmaf(F(3.0), F(5.0), F(-15.0)) == F(0.0)


# ---- geometry ------------------------------------------------------------------------------------------------------
def box(lo, hi):
    """closed axis-aligned box: 12 triangles [12][3][3]"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[lo[0] if not i & 1 else hi[0], lo[1] if not i & 2 else hi[1], lo[2] if not i & 4 else hi[2]] for i in range(8)])
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    tris = []
    for a, b, cc, d in quads:
        tris += [[c[a], c[b], c[cc]], [c[a], c[cc], c[d]]]
    return np.asarray(tris, np.float32)


class World:
    """triangles + per-triangle material and actor ids + the [M][B] tables, as the library and the oracle get them"""

    def __init__(self, parts, absorption, transmission=None, B=4):
        self.tri = np.concatenate([p[0] for p in parts]).astype(np.float32) if parts else np.zeros((0, 3, 3), np.float32)
        self.mat = np.concatenate([np.full(len(p[0]), p[1], np.uint16) for p in parts]) if parts else np.zeros(0, np.uint16)
        self.obj = np.concatenate([np.full(len(p[0]), p[2], np.uint32) for p in parts]) if parts else np.zeros(0, np.uint32)
        self.absorption = np.asarray(absorption, np.float32).reshape(-1, B)
        self.transmission = None if transmission is None else np.asarray(transmission, np.float32).reshape(-1, B)
        self.B = B

    def context(self, pkg, fast=False):
        ctx = pkg.Context(num_bands=self.B)
        ctx.set_scene(self.tri, self.mat, self.absorption, self.transmission, object_ids=self.obj if len(self.obj) else None, fast=fast)
        return ctx


class Yardstick:
    def __init__(self, oracle_mod, w, tri=None):
        self.w, self.B = w, w.B
        tri = w.tri if tri is None else tri
        self.sc = oracle_mod.Scene(tri, w.mat, w.absorption, transmission=w.transmission) if len(tri) else None
        self.tau = [self.sc.lobe_table(m)[0][2].copy() for m in range(w.absorption.shape[0])] if self.sc is not None else []
        self.queries = 0

    def closest(self, o, d, tmax):
        if self.sc is None:
            return None
        self.queries += 1
        hit, t, tri, _ = self.sc.trace_closest([float(x) for x in o], [float(x) for x in d], float(tmax), brute=True)
        return (F(t), tri) if hit else None

    def gains(self, tri):
        m = int(self.w.mat[tri])
        return self.tau[m] if m < len(self.tau) else np.zeros(self.B, np.float32)

    def chain(self, o, d, length, own_ids, max_surfaces, step):
        B, step = self.B, F(step)
        T, crossed, rem, o = [F(1.0)] * B, 0, F(length), [F(x) for x in o]
        for q in range(MAX_QUERIES):
            if not (rem > 0):
                return True, crossed, T
            h = self.closest(o, d, rem)
            if h is None:
                return True, crossed, T
            t, tri = h
            obj = int(self.w.obj[tri])
            if not (obj != NO_OBJECT and obj in own_ids):
                crossed += 1
                if crossed > max_surfaces:
                    return False, crossed, [F(0.0)] * B
                tau = self.gains(tri)
                T = [F(T[b] * F(tau[b])) for b in range(B)]
                if all(x == 0 for x in T):
                    return False, crossed, T
            adv = F(t + step)
            o = [fmaf(adv, d[i], o[i]) for i in range(3)]
            rem = F(rem - adv)
            if q + 1 == MAX_QUERIES:
                return False, crossed, [F(0.0)] * B
        raise AssertionError("unreachable")

    def samples(self, S, L, offsets, src_obj=NO_OBJECT, lis_obj=NO_OBJECT, **params):
        """per sample k: (valid, reached, crossed, T) — the pieces the row is made of (also what the float64 check compares)"""
        p = dict(DEFAULTS, **params)
        S, L, r = [F(x) for x in S], [F(x) for x in L], F(p["source_radius"])
        own = {i for i in (src_obj, lis_obj) if i != NO_OBJECT}
        n = 1 if r == 0 else p["samples"]
        out = []
        for k in range(n):
            u = [F(x) for x in offsets[k]]
            valid = k == 0 or self.chain(S, u, r, own, p["max_surfaces"], p["step"])[1] == 0
            if not valid:
                out.append((False, False, 0, None))
                continue
            pk = [F(S[i] + F(r * u[i])) for i in range(3)]
            e = [F(L[i] - pk[i]) for i in range(3)]
            ln = F(np.sqrt(F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2]))))
            if ln == 0:
                out.append((True, True, 0, [F(1.0)] * self.B))
                continue
            inv = F(F(1.0) / ln)
            d = [F(e[i] * inv) for i in range(3)]
            reached, crossed, T = self.chain(pk, d, F(ln - F(p["pullback"])), own, p["max_surfaces"], p["step"])
            out.append((True, reached, crossed, T))
        return out

    def row(self, S, L, offsets, src_obj=NO_OBJECT, lis_obj=NO_OBJECT, **params):
        p = dict(DEFAULTS, **params)
        S32, L32 = [F(x) for x in S], [F(x) for x in L]
        dx, dy, dz = [F(L32[i] - S32[i]) for i in range(3)]
        distance = F(np.sqrt(F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))))
        delay = F(F(distance / F(p["dist_divisor"])) / F(p["sound_speed"]))
        sm = self.samples(S, L, offsets, src_obj, lis_obj, **params)
        valid = [s for s in sm if s[0]]
        V = len(valid)
        free = sum(1 for s in valid if s[1] and s[2] == 0)
        tr = np.zeros(8, np.float32)
        for b in range(self.B):
            total = 0.0
            for s in valid:
                total += float(s[3][b])
            tr[b] = F(total / float(V))
        return dict(distance=distance, delay=delay, visibility=F(F(free) / F(V)), surfaces=sm[0][2], samples_valid=V, transmission=tr)


def assert_row(got, want, where=""):
    for k in ("distance", "delay", "visibility", "surfaces", "samples_valid"):
        assert got[k] == want[k], f"{where}: {k}: got {got[k]!r}, restatement {want[k]!r}"
    assert np.array_equal(got["transmission"], want["transmission"]), f"{where}: transmission {got['transmission']} != {want['transmission']}"


# ---- the scenes -----------------------------------------------------------------------------------------------------
ROOM = ([0.0, 0.0, 0.0], [1000.0, 800.0, 300.0])
ALPHA = [[0.5, 0.5, 0.5, 0.5], [0.6, 0.5, 0.7, 0.4], [0.9, 0.9, 0.9, 0.9], [1.0, 1.0, 1.0, 1.0]]
TAU = [[0.05, 0.1, 0.02, 0.0], [0.3, 0.25, 0.5, 0.4], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]]   # tau <= alpha: nothing is clamped
WALLS, SLAB, OPAQUE, CLEAR = 0, 1, 2, 3   # material ids; actor ids: the room 1, partitions 2, the own actor 7, the door 5
SRC, LIS = [250.0, 200.0, 150.0], [750.0, 600.0, 120.0]


def shoebox_world(extra=(), transmission=TAU):
    return World([(box(*ROOM), WALLS, 1)] + list(extra), ALPHA, transmission)


def partition_world(transmission=TAU):
    """a closed 10 cm slab across the room between source and listener"""
    return shoebox_world([(box([495.0, 1.0, 1.0], [505.0, 799.0, 299.0]), SLAB, 2)], transmission)


def half_wall_world():
    """a slab 40 cm from SRC whose edge (y = 250) lies beside the line to LIS: the source sphere (r = 50) sees round it in part"""
    return shoebox_world([(box([290.0, 1.0, 1.0], [300.0, 250.0, 299.0]), SLAB, 2)])


def offsets_of(pkg, n):
    return pkg.Context.direct_sample_offsets(n)


# ---- CPU: exports, bindings, offsets ----------------------------------------------------------------------------------
def test_struct_sizes_and_defaults(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.DirectParams) == 32 and C.sizeof(cap.DirectPath) == 52
    assert pkg.Context.DIRECT_DTYPE.itemsize == 52
    p = cap.default_direct_params()
    assert p.struct_size == 32
    assert (p.samples, p.max_surfaces) == (16, 8)
    assert p.source_radius == 0.0 and p.step == F(0.1) and p.pullback == F(0.1)
    assert p.dist_divisor == 1000.0 and p.sound_speed == 343.0
    assert (cap.MAX_DIRECT_BATCH, cap.MAX_DIRECT_SAMPLES, cap.DIRECT_MAX_QUERIES) == (256, 64, 32)
    for name in ("fs_direct_params_default", "fs_direct_sample_offsets", "fs_update_direct_paths"):
        assert name in cap.EXPORTS and hasattr(cap.load(), name)


def test_null_context_and_no_device(pkg):
    contract.null_context_and_no_device(pkg, QUERY)


@pytest.mark.parametrize("n", [1, 2, 3, 16, 64])
def test_sample_offsets(pkg, n):
    u = offsets_of(pkg, n)
    assert u.shape == (n, 3) and u.dtype == np.float32
    assert np.all(u[0] == 0)
    if n == 1:
        return
    j = np.arange(n - 1, dtype=np.float64)
    z = 1.0 - (2.0 * j + 1.0) / (n - 1)
    rho = np.sqrt(1.0 - z * z)
    phi = j * np.pi * (3.0 - np.sqrt(5.0))
    ref = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    ref32 = ref.astype(np.float32)
    ulp = np.maximum(np.spacing(np.abs(ref32)), np.spacing(np.abs(u[1:])))
    assert np.all(np.abs(u[1:].astype(np.float64) - ref) <= ulp.astype(np.float64)), "more than 1 float32 ulp from the formula"
    assert np.all(np.abs(np.linalg.norm(u[1:].astype(np.float64), axis=1) - 1.0) <= 2e-7)


def test_sample_offsets_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    buf = np.full((66, 3), 5.0, np.float32)
    assert lib.fs_direct_sample_offsets(0, buf.ctypes.data) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_direct_sample_offsets(65, buf.ctypes.data) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_direct_sample_offsets(-1, buf.ctypes.data) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_direct_sample_offsets(16, None) == cap.ERR_INVALID_ARGUMENT
    assert np.all(buf == 5.0)
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.direct_sample_offsets(65)


# ---- CPU: the yardstick against a float64 brute force -------------------------------------------------------------------
def crossings64(tri, o, d, length):
    """Moeller-Trumbore in double over all triangles: (t, triangle, margin) of every crossing with t in (0, length], sorted by t;
    marginal = some triangle's plane is met within a centimetre of the segment with a barycentric coordinate within 1e-4 of an
    edge, or at a grazing angle"""
    tri = tri.astype(np.float64)
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    p = np.cross(d, e2)
    det = np.einsum("ij,ij->i", e1, p)
    ok = np.abs(det) > 1e-12
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    s = o - v0
    u = np.einsum("ij,ij->i", s, p) * inv
    q = np.cross(s, e1)
    v = np.einsum("j,ij->i", d, q) * inv
    t = np.einsum("ij,ij->i", e2, q) * inv
    m = np.minimum(np.minimum(u, v), 1.0 - u - v)
    near = ok & (t > -1.0) & (t < length + 1.0)
    marginal = bool(np.any(near & (np.abs(m) < 1e-4)))
    hit = ok & (m > 0) & (t > 0) & (t <= length)
    idx = np.nonzero(hit)[0]
    idx = idx[np.argsort(t[idx])]
    ts = t[idx]
    if len(ts) and (ts[0] < 1.0 or length - ts[-1] < 1.0 or np.any(np.diff(ts) < 1.0)):
        marginal = True
    return [(float(t[i]), int(i)) for i in idx], marginal


def chain64(w, tau64, o, d, length, own, max_surfaces):
    cr, marginal = crossings64(w.tri, o, d, length)
    T, crossed = np.ones(w.B), 0
    for q, (_, i) in enumerate(cr):
        obj = int(w.obj[i])
        if not (obj != NO_OBJECT and obj in own):
            crossed += 1
            if crossed > max_surfaces:
                return False, crossed, np.zeros(w.B), marginal
            T = T * tau64[int(w.mat[i])]
            if np.all(T == 0):
                return False, crossed, T, marginal
        if q + 1 == MAX_QUERIES:
            return False, crossed, np.zeros(w.B), marginal
    return True, crossed, T, marginal


def samples64(w, tau64, S, L, offsets, r, max_surfaces=8, pullback=0.1):
    """(counts, valid, reached, crossed, T) per sample, everything in double"""
    S, L = np.asarray(S, np.float64), np.asarray(L, np.float64)
    out = []
    for k in range(len(offsets)):
        u = offsets[k].astype(np.float64)
        marg_a = False
        valid = True
        if k > 0:
            _, c, _, marg_a = chain64(w, tau64, S, u, r, set(), max_surfaces)
            valid = c == 0
        pk = S + r * u
        e = L - pk
        ln = float(np.linalg.norm(e))
        reached, crossed, T, marg_b = chain64(w, tau64, pk, e / ln, ln - pullback, set(), max_surfaces)
        out.append((not (marg_a or marg_b), valid, reached, crossed, T))
    return out


YARD_CASES = {
    # scene constants chosen so that the float64 reference alone meets the shares asserted below
    "partition": (partition_world, 30.0, [SRC, [120.0, 650.0, 60.0], [400.0, 330.0, 222.0], [47.0, 61.0, 250.0]]),
    "half_wall": (half_wall_world, 50.0, [SRC, [250.0, 215.0, 140.0], [246.0, 236.0, 170.0], [252.0, 260.0, 100.0]]),
}


@pytest.mark.parametrize("name", sorted(YARD_CASES))
def test_yardstick_against_float64_brute_force(pkg, oracle_mod, name):
    make, r, sources = YARD_CASES[name]
    w = make()
    y = Yardstick(oracle_mod, w)
    n = 33
    off = offsets_of(pkg, n)
    tau64 = np.minimum(np.maximum(w.transmission.astype(np.float64), 0.0), w.absorption.astype(np.float64))
    total = counted = valid64 = 0
    for S in sources:
        got = y.samples(S, LIS, off, samples=n, source_radius=r)
        ref = samples64(w, tau64, S, LIS, off, r)
        for k, (g, (counts, valid, reached, crossed, T)) in enumerate(zip(got, ref)):
            total += 1
            valid64 += bool(valid)
            if not counts:
                continue
            counted += 1
            where = f"{name} S={S} k={k}"
            assert g[0] == valid, where
            if not valid:
                continue
            assert g[2] == crossed, (where, g[2], crossed)
            assert (g[1] and g[2] == 0) == (reached and crossed == 0), where
            assert g[1] == reached, where
            assert np.allclose(np.asarray(g[3], np.float64), T, rtol=1e-6, atol=0.0), (where, g[3], T)
    assert total - counted <= 0.05 * total, f"{total - counted} of {total} samples are marginal in float64"
    assert valid64 >= 0.80 * total, f"only {valid64} of {total} samples are valid in float64"


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def check_rows(ctx, y, handles, positions, listener, off, where, src_obj=None, lis_obj=NO_OBJECT, **params):
    rows = ctx.direct_paths(handles, **params)
    for i, S in enumerate(positions):
        so = NO_OBJECT if src_obj is None else src_obj[i]
        assert_row(rows[i], y.row(S, listener, off, so, lis_obj, **params), f"{where} row {i}")
    return rows


@pytest.mark.gpu
def test_free_line(pkg, oracle_mod):
    w = shoebox_world()
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    y = Yardstick(oracle_mod, w)
    h = place(ctx, [SRC, LIS])
    rows = check_rows(ctx, y, h, [SRC, LIS], LIS, offsets_of(pkg, 1), "free", samples=1)
    assert rows[0]["visibility"] == 1 and rows[0]["surfaces"] == 0 and rows[0]["samples_valid"] == 1
    assert np.array_equal(rows[0]["transmission"], np.array([1, 1, 1, 1, 0, 0, 0, 0], np.float32))
    d = [F(LIS[i]) - F(SRC[i]) for i in range(3)]
    dist = np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    assert rows[0]["distance"] == dist and rows[0]["delay"] == F(F(dist / F(1000.0)) / F(343.0))
    assert rows[1]["distance"] == 0 and rows[1]["delay"] == 0 and rows[1]["visibility"] == 1
    assert np.array_equal(rows[1]["transmission"][:4], np.ones(4, np.float32))
    # a point source ignores `samples`; a sphere in free air sees all of itself
    assert ctx.direct_paths(h, samples=16).tobytes() == rows.tobytes()
    rows = check_rows(ctx, y, h[:1], [SRC], LIS, offsets_of(pkg, 16), "free sphere", samples=16, source_radius=30.0)
    assert rows[0]["visibility"] == 1 and rows[0]["samples_valid"] == 16
    ctx.close()
    # an empty committed scene: free lines
    e = World([], ALPHA, TAU)
    ctx = e.context(pkg)
    ctx.set_listener(LIS)
    rows = check_rows(ctx, Yardstick(oracle_mod, e), place(ctx, [SRC]), [SRC], LIS, offsets_of(pkg, 16), "empty", samples=16, source_radius=30.0)
    assert rows[0]["visibility"] == 1 and rows[0]["samples_valid"] == 16 and rows[0]["transmission"][0] == 1
    ctx.close()


@pytest.mark.gpu
def test_partition(pkg, oracle_mod):
    w = partition_world()
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows = check_rows(ctx, Yardstick(oracle_mod, w), h, [SRC], LIS, offsets_of(pkg, 1), "partition", samples=1)
    assert rows[0]["surfaces"] == 2 and rows[0]["visibility"] == 0
    tau = np.asarray(TAU[SLAB], np.float32)
    assert np.array_equal(rows[0]["transmission"][:4], tau * tau)
    assert np.all(rows[0]["transmission"][4:] == 0)
    ctx.close()
    w = partition_world(transmission=None)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows = check_rows(ctx, Yardstick(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, offsets_of(pkg, 1), "no transmission array", samples=1)
    assert np.all(rows[0]["transmission"] == 0) and rows[0]["surfaces"] == 1 and rows[0]["visibility"] == 0
    ctx.close()


@pytest.mark.gpu
def test_half_covered_source(pkg, oracle_mod):
    w = half_wall_world()
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    y = Yardstick(oracle_mod, w)
    n = 33
    pos = [SRC, [250.0, 215.0, 140.0], [246.0, 236.0, 170.0], [20.0, 400.0, 150.0]]   # the last: 20 cm from the x = 0 wall
    rows = check_rows(ctx, y, place(ctx, pos), pos, LIS, offsets_of(pkg, n), "half wall", samples=n, source_radius=50.0)
    assert 0 < rows[0]["visibility"] < 1
    assert rows[3]["samples_valid"] < n
    ctx.close()


_rooms = {}


def rooms_case(pkg, oracle_mod):
    """starter_room with synthetic lobes, 64 seeded sources, and the restatement's rows — computed once"""
    if not _rooms:
        sc = pkg.scenes.starter_room(4)
        tr, _ = pkg.scenes.material_lobes(sc)
        w = World([], sc.absorption, tr)
        w.tri, w.mat, w.obj = sc.triangles.astype(np.float32), sc.material_ids.astype(np.uint16), sc.object_ids.astype(np.uint32)
        rng = np.random.default_rng(0xD1EC7)
        lo, hi = w.tri.reshape(-1, 3).min(axis=0), w.tri.reshape(-1, 3).max(axis=0)
        pos = rng.uniform(lo, hi, (64, 3)).astype(np.float32)
        params = dict(samples=16, source_radius=30.0)
        y = Yardstick(oracle_mod, w)
        off = offsets_of(pkg, 16)
        lis = sc.listener
        _rooms.update(w=w, pos=pos, lis=lis, params=params, want=[y.row(S, lis, off, **params) for S in pos])
    return _rooms


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["sah", "device_morton"])
def test_rooms(pkg, oracle_mod, fast):
    rc = rooms_case(pkg, oracle_mod)
    ctx = rc["w"].context(pkg, fast=fast)
    ctx.set_listener(rc["lis"])
    h = place(ctx, rc["pos"])
    rows = ctx.direct_paths(h, **rc["params"])
    for i in range(64):
        assert_row(rows[i], rc["want"][i], f"rooms fast={fast} row {i}")
    assert len({r["visibility"] for r in rows}) > 2 and any(0 < r["transmission"][0] < 1 for r in rows)   # the case is not trivial
    one = np.concatenate([ctx.direct_paths([x], **rc["params"]) for x in h])
    assert one.tobytes() == rows.tobytes(), "count = 64 differs from 64 calls with count = 1"
    twice = ctx.direct_paths([h[5], h[9], h[5]], **rc["params"])
    assert twice[0].tobytes() == rows[5].tobytes() == twice[2].tobytes() and twice[1].tobytes() == rows[9].tobytes()
    ctx.close()


@pytest.mark.gpu
def test_own_actors(pkg, oracle_mod):
    wall = (box([495.0, 1.0, 1.0], [505.0, 799.0, 299.0]), SLAB, 2)
    off = offsets_of(pkg, 16)
    params = dict(samples=16, source_radius=5.0)
    bare = shoebox_world([wall])
    ctx = bare.context(pkg)
    ctx.set_listener(LIS)
    want = ctx.direct_paths(place(ctx, [SRC]), **params)
    assert_row(want[0], Yardstick(oracle_mod, bare).row(SRC, LIS, off, **params), "bare")
    ctx.close()
    for side, centre in (("source", SRC), ("listener", LIS)):
        c = np.asarray(centre)
        w = shoebox_world([wall, (box(c - 20.0, c + 20.0), OPAQUE, 7)])
        y = Yardstick(oracle_mod, w)
        ctx = w.context(pkg)
        ctx.set_listener(LIS)
        h = place(ctx, [SRC])
        rows = check_rows(ctx, y, h, [SRC], LIS, off, f"{side} boxed", **params)
        assert rows[0]["visibility"] == 0 and np.all(rows[0]["transmission"] == 0) and rows[0]["surfaces"] == (1 if side == "source" else 3)
        if side == "source":
            ctx.set_source_object(h[0], 7)
            rows = check_rows(ctx, y, h, [SRC], LIS, off, "source owns the box", src_obj=[7], **params)
        else:
            ctx.set_listener_object(7)
            rows = check_rows(ctx, y, h, [SRC], LIS, off, "listener owns the box", lis_obj=7, **params)
        assert rows.tobytes() == want.tobytes(), f"{side}: not the result of the scene without the box"
        ctx.close()


def slabs_world(count):
    pitch = 700.0 / count
    return shoebox_world([(box([150.0 + pitch * i, 1.0, 1.0], [160.0 + pitch * i, 799.0, 299.0]), CLEAR, 2) for i in range(count)])


@pytest.mark.gpu
def test_caps(pkg, oracle_mod):
    S, L = [100.0, 400.0, 150.0], [900.0, 410.0, 140.0]
    off = offsets_of(pkg, 1)
    w = slabs_world(5)
    ctx = w.context(pkg)
    ctx.set_listener(L)
    y = Yardstick(oracle_mod, w)
    h = place(ctx, [S])
    rows = check_rows(ctx, y, h, [S], L, off, "5 slabs, 4 allowed", samples=1, max_surfaces=4)
    assert np.all(rows[0]["transmission"] == 0) and rows[0]["surfaces"] == 5
    rows = check_rows(ctx, y, h, [S], L, off, "5 slabs, 16 allowed", samples=1, max_surfaces=16)
    assert np.array_equal(rows[0]["transmission"][:4], np.ones(4, np.float32)) and rows[0]["surfaces"] == 10 and rows[0]["visibility"] == 0
    ctx.close()
    w = slabs_world(20)
    ctx = w.context(pkg)
    ctx.set_listener(L)
    y, h = Yardstick(oracle_mod, w), place(ctx, [S])
    rows = check_rows(ctx, y, h, [S], L, off, "20 slabs", samples=1, max_surfaces=31)
    assert np.all(rows[0]["transmission"] == 0) and rows[0]["visibility"] == 0 and rows[0]["surfaces"] == 32
    # as the source's own actor the 40 surfaces count for nothing, but the 32nd query in a row still ends the ray
    ctx.set_source_object(h[0], 2)
    rows = check_rows(ctx, y, h, [S], L, off, "20 own slabs", src_obj=[2], samples=1, max_surfaces=31)
    assert np.all(rows[0]["transmission"] == 0) and rows[0]["visibility"] == 0 and rows[0]["surfaces"] == 0
    ctx.close()


@pytest.mark.gpu
def test_movers(pkg, oracle_mod):
    door = box([495.0, 300.0, 1.0], [505.0, 500.0, 250.0])
    w = shoebox_world([(door, OPAQUE, 5)])
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    off = offsets_of(pkg, 16)
    params = dict(samples=16, source_radius=20.0)
    rows = check_rows(ctx, Yardstick(oracle_mod, w), h, [SRC], LIS, off, "door shut", **params)
    assert rows[0]["visibility"] == 0 and rows[0]["surfaces"] == 1
    aside = np.array([[1, 0, 0, 0], [0, 1, 0, 350], [0, 0, 1, 0]], np.float32)
    ctx.set_object_transforms([5], aside[None])
    rows = check_rows(ctx, Yardstick(oracle_mod, w, contract.transformed(w, 5, aside)), h, [SRC], LIS, off, "door aside, no explicit refit", **params)   # the call refits first
    assert rows[0]["visibility"] == 1 and rows[0]["surfaces"] == 0 and rows[0]["transmission"][0] == 1
    ctx.set_object_transforms([5], np.eye(3, 4, dtype=np.float32)[None])
    rows = check_rows(ctx, Yardstick(oracle_mod, w), h, [SRC], LIS, off, "door back", **params)
    assert rows[0]["visibility"] == 0
    ctx.close()


def _defaults_found(t, oracle_mod, want):
    assert want[0][0]["surfaces"] == 2


inf, nan = float("inf"), float("nan")
QUERY = contract.Query(
    kind="direct", dtypes=("DIRECT_DTYPE",), world=partition_world, src=SRC, lis=LIS, wrong_struct_size=28,
    refused=(dict(samples=0), dict(samples=65), dict(source_radius=-1.0), dict(source_radius=inf), dict(source_radius=nan),
             dict(max_surfaces=0), dict(max_surfaces=32), dict(step=-0.1), dict(step=nan), dict(step=inf), dict(pullback=-1.0),
             dict(pullback=nan), dict(pullback=inf), dict(dist_divisor=0.0), dict(dist_divisor=-1.0), dict(dist_divisor=nan),
             dict(dist_divisor=inf), dict(sound_speed=0.0), dict(sound_speed=nan), dict(sound_speed=inf)),
    defaults_found=_defaults_found, legal=(dict(samples=64, source_radius=1.0, max_surfaces=31, step=0.0, pullback=0.0),),
    untouched=contract.DIRECT_SPHERE, steady=contract.DIRECT_SPHERE)


@pytest.mark.gpu
def test_errors_and_untouched_state(pkg):
    contract.errors_and_untouched_state(pkg, None, QUERY)


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    contract.steady_state_allocates_nothing(pkg, QUERY)


@pytest.mark.gpu
def test_component_layer(pkg, oracle_mod):
    """FrequenSeeAudioComponent.GetDirectPath and AudioRayTracingSubsystem.UpdateDirectPaths are the same call"""
    w = partition_world()
    sub = pkg.AudioRayTracingSubsystem(num_bands=4)
    sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
    sub.SetMaterials(w.absorption, w.transmission)
    comps = [pkg.FrequenSeeAudioComponent(p) for p in (SRC, [700.0, 100.0, 50.0])]
    for c in comps:
        c.OnRegister(sub)
    sub.SetListenerLocation(LIS)
    rows = sub.UpdateDirectPaths(samples=16, source_radius=30.0)
    y = Yardstick(oracle_mod, w)
    off = offsets_of(pkg, 16)
    for i, c in enumerate(comps):
        assert_row(rows[i], y.row(c.GetComponentLocation(), LIS, off, samples=16, source_radius=30.0), f"component {i}")
        assert c.GetDirectPath(samples=16, source_radius=30.0).tobytes() == rows[i].tobytes()
    assert rows[0]["surfaces"] == 2 and rows[1]["surfaces"] == 0
    sub.Deinitialize()
