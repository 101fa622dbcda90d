"""fs_update_reflection_paths: the first-order specular reflections of every source of a tick.

The yardstick is a Python restatement of include/frequensee.h's "reflection paths" rule on numpy float32 (every operation
rounded on its own, fmaf exact): the filter over all triangles as float32 array arithmetic, the two legs per candidate as
scalars.  Each closest hit comes from oracle.Scene.trace_closest(brute=True), the scan tests/test_gpu_parity.py holds the GPU
line trace to bit for bit; the records from the test's own vertices; the reflectance from Scene.lobe_table(m)[0][1] of the test's
own tables; the pass-through rule from the test's own object ids.  Every field of every row and path must EQUAL it, floats by bit
pattern.  The restatement itself is checked without a GPU against the float64 image-source construction in a shoebox whose
reflection points are, by assertion, nowhere near a triangle edge.
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

pytest.register_assert_rewrite("path_query_contract")
import path_query_contract as contract  # noqa: E402
from path_query_contract import assert_equal  # noqa: E402
from path_query_contract import device_free_bytes, place  # noqa: E402,F401  (other test files import them from here)

F = np.float32
NO_OBJECT = 0xFFFFFFFF
NO_MATERIAL = 0xFFFF
MAX_QUERIES = 32
DEFAULTS = dict(max_paths=8, max_candidates=256, margin=1e-3, step=0.1, offset=0.1, pullback=0.1, dist_divisor=1000.0, sound_speed=343.0)
FREE, TARGET, BLOCKED = 0, 1, 2


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


def dot(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z on float32 scalars or on [T][3] float32 arrays"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    """product, product, subtract per component"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


# ---- geometry ------------------------------------------------------------------------------------------------------
def quad_grid(origin, du, dv, n):
    """a parallelogram cut n x n, two triangles per cell, the cell's diagonal from its (0, 0) to its (1, 1) corner"""
    o, du, dv = (np.asarray(x, np.float64) for x in (origin, du, dv))
    tris = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = (o + du * (i + p) / n + dv * (j + q) / n for p, q in ((0, 0), (1, 0), (1, 1), (0, 1)))
            tris += [[a, b, c], [a, c, d]]
    return tris


def box(lo, hi, n=1):
    """closed axis-aligned box, every wall cut n x n: 12 n^2 triangles [.][3][3]; wall w (0 .. 5 = x lo, x hi, y lo, y hi, z lo,
    z hi) owns the triangles [2 n^2 w, 2 n^2 (w + 1))"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    tris = []
    for axis in range(3):
        u, v = [(1, 2), (0, 2), (0, 1)][axis]
        for side in (lo, hi):
            o = lo.copy()
            o[axis] = side[axis]
            du, dv = np.zeros(3), np.zeros(3)
            du[u], dv[v] = ext[u], ext[v]
            tris += quad_grid(o, du, dv, n)
    return np.asarray(tris, np.float32)


class World:
    """triangles + per-triangle material and actor ids + the [M][B] tables, as the library and the oracle get them"""

    def __init__(self, parts, absorption, transmission=None, B=4, scattering=None):
        self.tri = np.concatenate([np.asarray(p[0], np.float32).reshape(-1, 3, 3) for p in parts]) if parts else np.zeros((0, 3, 3), np.float32)
        self.mat = np.concatenate([np.full(len(p[0]), p[1], np.uint16) for p in parts]) if parts else np.zeros(0, np.uint16)
        self.obj = np.concatenate([np.full(len(p[0]), p[2], np.uint32) for p in parts]) if parts else np.zeros(0, np.uint32)
        self.absorption = np.asarray(absorption, np.float32).reshape(-1, B)
        self.transmission = None if transmission is None else np.asarray(transmission, np.float32).reshape(-1, B)
        self.scattering = None if scattering is None else np.asarray(scattering, np.float32).reshape(-1, B)
        self.B = B

    def context(self, pkg, fast=False):
        ctx = pkg.Context(num_bands=self.B)
        ctx.set_scene(self.tri, self.mat, self.absorption, self.transmission, self.scattering, object_ids=self.obj if len(self.obj) else None, fast=fast)
        return ctx


class Restatement:
    def __init__(self, oracle_mod, w, tri=None):
        self.w, self.B = w, w.B
        tri = (w.tri if tri is None else tri).astype(np.float32)
        self.sc = oracle_mod.Scene(tri, w.mat, w.absorption, transmission=w.transmission, scattering=w.scattering) if len(tri) else None
        self.spec = [self.sc.lobe_table(m)[0][1].copy() for m in range(w.absorption.shape[0])] if self.sc is not None else []
        self.v0, self.e1, self.e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]   # the records: one fp32 subtraction per component
        self.stats = dict(leg1_blocked=0, leg2_blocked=0, passed_own=0)

    def closest(self, o, d, tmax):
        hit, t, tri, _ = self.sc.trace_closest([float(x) for x in o], [float(x) for x in d], float(tmax), brute=True)
        return (F(t), tri) if hit else None

    def candidates(self, S, L, own, margin):
        """step 1 over all triangles at once: (input indices of the triangles that pass, ascending; D [T][3])"""
        T = len(self.v0)
        if T == 0:
            return np.zeros(0, np.int64), np.zeros((0, 3), np.float32)
        S, L, m = np.asarray(S, np.float32), np.asarray(L, np.float32), F(margin)
        with np.errstate(all="ignore"):
            n = cross(self.e1, self.e2)
            nn = dot(n, n)
            tv = L[None, :] - self.v0
            hS, hL = dot(S[None, :] - self.v0, n), dot(tv, n)
            side = ((hS > 0) & (hL > 0)) | ((hS < 0) & (hL < 0))
            k = (F(2.0) * hS) / nn
            D = (S[None, :] - k[:, None] * n) - L[None, :]
            p = cross(D, self.e2)
            det = dot(self.e1, p)
            inv = F(1.0) / det
            u = dot(tv, p) * inv
            q = cross(tv, self.e1)
            v = dot(D, q) * inv
            s = dot(self.e2, q) * inv
            ok = (nn != 0) & side & (det != 0) & (u >= -m) & (v >= -m) & ((u + v) <= F(1.0) + m) & (s > 0) & (s < 1)
        assert D.dtype == np.float32 and u.dtype == np.float32
        is_own = np.array([int(o) != NO_OBJECT and int(o) in own for o in self.w.obj], bool) if own else np.zeros(T, bool)
        return np.nonzero(ok & ~is_own)[0], D

    def leg(self, o, d, length, own, target, step):
        """(status, t1, P): passes own actors, ends at the first other triangle (TARGET if it is `target`) or free within length"""
        step, rem, acc, o = F(step), F(length), F(0.0), [F(x) for x in o]
        for q in range(MAX_QUERIES):
            if not (rem > 0):
                return FREE, None, None
            h = self.closest(o, d, rem)
            if h is None:
                return FREE, None, None
            t, tri = h
            obj = int(self.w.obj[tri])
            if not (obj != NO_OBJECT and obj in own):
                if tri == target:
                    return TARGET, F(acc + t), [fmaf(t, d[i], o[i]) for i in range(3)]
                return BLOCKED, None, None
            self.stats["passed_own"] += 1
            adv = F(t + step)
            o = [fmaf(adv, d[i], o[i]) for i in range(3)]
            rem = F(rem - adv)
            acc = F(acc + adv)
        return BLOCKED, None, None

    def reflectance(self, tri):
        m, r = int(self.w.mat[tri]), np.zeros(8, np.float32)
        r[:self.B] = self.spec[m] if m != NO_MATERIAL and m < len(self.spec) else F(1.0)
        return r

    def row(self, S, L, src_obj=NO_OBJECT, lis_obj=NO_OBJECT, **params):
        """(row dict, confirmed paths in the rule's order: all of them, not only max_paths)"""
        p = dict(DEFAULTS, **params)
        S32, L32 = [F(x) for x in S], [F(x) for x in L]
        own = {i for i in (src_obj, lis_obj) if i != NO_OBJECT}
        cand, D = self.candidates(S32, L32, own, p["margin"])
        if len(cand) > p["max_candidates"]:
            return dict(candidates=len(cand), found=0, returned=0, flags=1), []
        paths = []
        for i in cand:
            Di = D[i]
            len1 = F(np.sqrt(dot(Di, Di)))
            with np.errstate(all="ignore"):
                inv = F(1.0) / len1
            d = [F(Di[k] * inv) for k in range(3)]
            status, t1, P = self.leg(L32, d, len1, own, int(i), p["step"])
            if status != TARGET:
                self.stats["leg1_blocked"] += 1
                continue
            e = np.array([F(S32[k] - P[k]) for k in range(3)], np.float32)
            len2 = F(np.sqrt(dot(e, e)))
            if len2 == 0:
                continue
            inv2 = F(1.0) / len2
            d2 = [F(e[k] * inv2) for k in range(3)]
            o2 = [fmaf(F(p["offset"]), d2[k], P[k]) for k in range(3)]
            status, _, _ = self.leg(o2, d2, F(F(len2 - F(p["offset"])) - F(p["pullback"])), own, -1, p["step"])
            if status != FREE:
                self.stats["leg2_blocked"] += 1
                continue
            length = F(t1 + len2)
            paths.append(dict(length=length, delay=F(F(length / F(p["dist_divisor"])) / F(p["sound_speed"])), point=np.array(P, np.float32),
                              direction=np.array(d, np.float32), triangle=int(i), material=int(self.w.mat[i]), reflectance=self.reflectance(i)))
        paths.sort(key=lambda x: (bits(x["length"]), x["triangle"]))
        return dict(candidates=len(cand), found=len(paths), returned=min(len(paths), p["max_paths"]), flags=0), paths

    def expect(self, pkg, positions, L, src_obj=None, lis_obj=NO_OBJECT, **params):
        """the call's two arrays as the library must write them"""
        mp = dict(DEFAULTS, **params)["max_paths"]
        rows = np.zeros(len(positions), dtype=pkg.Context.REFLECTION_ROW_DTYPE)
        paths = np.zeros((len(positions), mp), dtype=pkg.Context.REFLECTION_DTYPE)
        for i, S in enumerate(positions):
            r, ps = self.row(S, L, NO_OBJECT if src_obj is None else src_obj[i], lis_obj, **params)
            for k in rows.dtype.names:
                rows[i][k] = r[k]
            for j, x in enumerate(ps[:mp]):
                for k in paths.dtype.names:
                    paths[i, j][k] = x[k]
        return rows, paths


# ---- the scenes -----------------------------------------------------------------------------------------------------
LO, HI = [0.0, 0.0, 0.0], [1000.0, 800.0, 300.0]
ALPHA = [[0.5, 0.4, 0.3, 0.2], [0.6, 0.5, 0.7, 0.4], [0.9, 0.9, 0.9, 0.9], [1.0, 1.0, 1.0, 1.0]]
TAU = [[0.05, 0.1, 0.02, 0.0], [0.3, 0.25, 0.5, 0.4], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]]
SCAT = [[0.2, 0.3, 0.4, 0.5], [0.1, 0.6, 0.3, 0.9], [0.5, 0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0]]   # (no scattering array: nothing specular)
WALLS, SLAB, OPAQUE = 0, 1, 2   # material ids; actor ids: the room 1, partitions 2, the door 5, own actors 7 and 8
SRC, LIS = [310.0, 230.0, 170.0], [720.0, 560.0, 110.0]


def shoebox_world(extra=(), n=1):
    return World([(box(LO, HI, n), WALLS, 1)] + list(extra), ALPHA, TAU, 4, SCAT)


def image_source(S, L, wall):
    """float64: (|mirror(S) - L|, the reflection point) for wall 0 .. 5 of the room"""
    S, L = np.asarray(S, np.float64), np.asarray(L, np.float64)
    axis, plane = wall // 2, (LO, HI)[wall % 2][wall // 2]
    M = S.copy()
    M[axis] = 2.0 * plane - S[axis]
    s = (plane - L[axis]) / (M[axis] - L[axis])
    return float(np.linalg.norm(M - L)), L + s * (M - L)


def margin64(tri, P):
    """float64: the largest min(u, v, 1 - u - v) of P over the triangles whose plane it lies in (the triangle P is in, and how deep)"""
    tri = tri.astype(np.float64)
    best, arg = -np.inf, -1
    for i, (a, b, c) in enumerate(tri):
        e1, e2, r = b - a, c - a, P - a
        n = np.cross(e1, e2)
        if abs(np.dot(r, n)) > 1e-9 * np.dot(n, n) ** 0.5 * 1000.0:
            continue
        u, v = np.dot(np.cross(r, e2), n) / np.dot(n, n), np.dot(np.cross(e1, r), n) / np.dot(n, n)
        m = min(u, v, 1.0 - u - v)
        if m > best:
            best, arg = m, i
    return best, arg


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.ReflectionParams) == 36 and C.sizeof(cap.ReflectionPath) == 72 and C.sizeof(cap.ReflectionRow) == 16
    assert pkg.Context.REFLECTION_DTYPE.itemsize == 72 and pkg.Context.REFLECTION_ROW_DTYPE.itemsize == 16
    p = cap.default_reflection_params()
    assert p.struct_size == 36
    assert (p.max_paths, p.max_candidates) == (8, 256)
    assert p.margin == F(1e-3) and p.step == F(0.1) and p.offset == F(0.1) and p.pullback == F(0.1)
    assert p.dist_divisor == 1000.0 and p.sound_speed == 343.0
    assert (cap.MAX_REFLECTIONS, cap.MAX_REFLECTION_CANDIDATES, cap.MAX_REFLECTION_BATCH, cap.REFLECTION_OVERFLOW) == (16, 256, 256, 1)


def test_exported_in_one_tier(pkg):
    contract.exported_in_one_tier(pkg, ("fs_reflection_params_default", "fs_update_reflection_paths"))


def test_null_context_and_no_device(pkg):
    contract.null_context_and_no_device(pkg, QUERY)


@pytest.mark.parametrize("n", [1, 4], ids=["12_triangles", "192_triangles"])
def test_restatement_against_image_sources(pkg, oracle_mod, n):
    """S and L are chosen so that, in float64, every reflection point lies more than 1e-2 (barycentric) inside its triangle and no
    two lengths are closer than 1e-3 relative: six reflections, one per wall, are a property of the input, not of rounding"""
    w = shoebox_world(n=n)
    per_wall = 2 * n * n
    assert len(w.tri) == 6 * per_wall
    want = [image_source(SRC, LIS, wall) for wall in range(6)]
    for wall, (_, P) in enumerate(want):
        m, tri = margin64(w.tri, P)
        assert m > 1e-2, f"wall {wall}: reflection point only {m} inside its triangle"
        assert tri // per_wall == wall
    lengths = sorted(x[0] for x in want)
    assert all((b - a) / b > 1e-3 for a, b in zip(lengths, lengths[1:]))
    y = Restatement(oracle_mod, w)
    r, paths = y.row(SRC, LIS)
    assert r == dict(candidates=6, found=6, returned=6, flags=0)
    assert sorted(p["triangle"] // per_wall for p in paths) == list(range(6))
    assert [bits(p["length"]) for p in paths] == sorted(bits(p["length"]) for p in paths)
    size = float(np.max(np.asarray(HI) - np.asarray(LO)))
    for p in paths:
        wall = p["triangle"] // per_wall
        ref, P = want[wall]
        # the chain is about twenty fp32 roundings of 6e-8 each: 1e-5 leaves nearly an order of magnitude
        assert abs(float(p["length"]) - ref) <= 1e-5 * ref, (wall, p["length"], ref)
        axis = wall // 2
        assert abs(float(p["point"][axis]) - (LO, HI)[wall % 2][axis]) <= 1e-5 * size, (wall, p["point"])
        assert margin64(w.tri, P)[1] == p["triangle"]
        assert np.allclose(p["point"], P, rtol=0, atol=1e-5 * size * 10)
        assert np.array_equal(p["reflectance"][:4], y.spec[WALLS]) and np.all(p["reflectance"][4:] == 0)
        assert np.all((p["reflectance"][:4] > 0) & (p["reflectance"][:4] < 1))


# ---- GPU ---------------------------------------------------------------------------------------------------------------
check = contract.checker("reflection")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4], ids=["12_triangles", "192_triangles"])
def test_shoebox(pkg, oracle_mod, n):
    w = shoebox_world(n=n)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Restatement(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, f"shoebox n={n}")
    assert tuple(rows[0]) == (6, 6, 6, 0)
    assert sorted(int(t) // (2 * n * n) for t in paths[0]["triangle"][:6]) == list(range(6))
    assert np.all(paths[0][6:].view(np.uint8) == 0)
    ctx.close()


@pytest.mark.gpu
def test_shared_edge_and_equal_lengths(pkg, oracle_mod):
    w = shoebox_world()
    y = Restatement(oracle_mod, w)
    ctx = w.context(pkg)
    # mirror-symmetric about the floor's and the ceiling's diagonal (0, 0) - (1000, 800), at one height: those two reflection points
    # lie on the edge the wall's two triangles share.  Only equality is asserted: either triangle, both or none may claim the point.
    a = np.array([1000.0, 800.0]) / np.hypot(1000.0, 800.0)
    s2 = np.array([430.0, 180.0])
    l2 = 2.0 * np.dot(s2, a) * a - s2
    S, L = [s2[0], s2[1], 140.0], [l2[0], l2[1], 140.0]
    ctx.set_listener(L)
    check(pkg, ctx, y, place(ctx, [S]), [S], L, "shared edge")
    # source and listener at the centre: opposite walls give equal lengths, the triangle index decides; every reflection point is
    # the centre of a wall, on its diagonal
    centre = [500.0, 400.0, 150.0]
    ctx.set_listener(centre)
    check(pkg, ctx, y, place(ctx, [centre, [500.0, 400.0, 100.0]]), [centre, [500.0, 400.0, 100.0]], centre, "centre")
    ctx.close()


@pytest.mark.gpu
def test_blocked_legs(pkg, oracle_mod):
    # a partition across most of the room between source and listener, and a half wall beside the listener
    w = shoebox_world([(box([495.0, 1.0, 1.0], [505.0, 600.0, 299.0]), SLAB, 2), (box([600.0, 300.0, 1.0], [610.0, 799.0, 200.0]), OPAQUE, 2)])
    y = Restatement(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    pos = [SRC, [120.0, 650.0, 60.0], [400.0, 330.0, 222.0], [650.0, 700.0, 250.0], [560.0, 100.0, 40.0], [650.0, 300.0, 150.0]]
    rows, paths = check(pkg, ctx, y, place(ctx, pos), pos, LIS, "blocked legs")
    assert y.stats["leg1_blocked"] > 0 and y.stats["leg2_blocked"] > 0, y.stats
    assert len(set(rows["found"])) > 1 and np.any(rows["found"] < rows["candidates"])
    assert np.any(paths["triangle"] >= 12), "no reflection off the partitions"
    ctx.close()


@pytest.mark.gpu
def test_own_actors(pkg, oracle_mod):
    s, l = np.asarray(SRC), np.asarray(LIS)
    w = shoebox_world([(box(s - 25.0, s + 25.0), OPAQUE, 8), (box(l - 30.0, l + 30.0), OPAQUE, 7)])
    bare = shoebox_world()
    ctx = bare.context(pkg)
    ctx.set_listener(LIS)
    want = check(pkg, ctx, Restatement(oracle_mod, bare), place(ctx, [SRC]), [SRC], LIS, "bare")
    ctx.close()
    y = Restatement(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    # foreign ids: the two meshes block every leg (both ends are boxed in) and reflect what starts inside them
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "foreign meshes")
    assert rows[0]["candidates"] > 6, "no face of the meshes is a candidate"
    assert not np.any(paths[0]["triangle"][:rows[0]["returned"]] < 12), "a wall was reached through a closed box"
    ctx.set_source_object(h[0], 8)
    ctx.set_listener_object(7)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "own meshes", src_obj=[8], lis_obj=7)
    assert y.stats["passed_own"] > 0
    assert tuple(rows[0]) == (6, 6, 6, 0) and np.all(paths[0]["triangle"][:6] < 12), "an own mesh reflected or blocked"
    # the legs step past the own surfaces, so the lengths may differ from the bare room's in the last bits; the reflectors do not
    assert np.array_equal(paths[0]["triangle"], want[1][0]["triangle"])
    ctx.close()


@pytest.mark.gpu
def test_caps(pkg, oracle_mod):
    w = shoebox_world()
    y = Restatement(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    full = ctx.reflection_paths(h)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "three shortest", max_paths=3)
    assert tuple(rows[0]) == (6, 6, 3, 0) and paths.shape == (1, 3)
    assert paths[0].tobytes() == full[1][0][:3].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "overflow", max_candidates=2)
    assert tuple(rows[0]) == (6, 0, 0, pkg._capi.REFLECTION_OVERFLOW)
    assert np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "exactly the cap", max_candidates=6, max_paths=16)
    assert tuple(rows[0]) == (6, 6, 6, 0) and paths.shape == (1, 16)
    ctx.close()


@pytest.mark.gpu
def test_materials_and_degenerate_triangles(pkg, oracle_mod):
    room = box(LO, HI)
    degenerate = np.array([[[0.0, 100.0, 100.0], [0.0, 100.0, 100.0], [0.0, 300.0, 200.0]],      # two corners equal
                           [[100.0, 0.0, 50.0], [300.0, 0.0, 150.0], [500.0, 0.0, 250.0]],       # three on a line
                           [[400.0, 300.0, 0.0], [400.0, 300.0, 0.0], [400.0, 300.0, 0.0]]], np.float32)   # a point
    # walls x: material 0; walls y: no material; walls z: an id beyond the table; three bands
    w = World([(room[0:4], 0, 1), (room[4:8], NO_MATERIAL, 1), (room[8:12], 9, 1), (degenerate, 0, 1)], [a[:3] for a in ALPHA], [t[:3] for t in TAU], 3, [x[:3] for x in SCAT])
    y = Restatement(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, y, place(ctx, [SRC]), [SRC], LIS, "materials")
    assert tuple(rows[0]) == (6, 6, 6, 0)
    for p in paths[0][:6]:
        assert p["triangle"] < 12 and p["material"] == w.mat[p["triangle"]]
        assert np.all(p["reflectance"][3:] == 0)
        if p["material"] == 0:
            assert np.array_equal(p["reflectance"][:3], y.spec[0]) and np.all((p["reflectance"][:3] > 0) & (p["reflectance"][:3] < 1))
        else:
            assert np.all(p["reflectance"][:3] == 1)
    for k in ("length", "delay", "point", "direction", "reflectance"):
        assert np.all(np.isfinite(paths[k]))
    ctx.close()


_rooms = {}


def rooms_case(pkg, oracle_mod):
    """starter_room with synthetic lobes, 64 seeded sources, and the restatement's arrays — computed once"""
    if not _rooms:
        sc = pkg.scenes.starter_room(4)
        tr, sca = pkg.scenes.material_lobes(sc)
        w = World([], sc.absorption, tr, 4, sca)
        w.tri, w.mat, w.obj = sc.triangles.astype(np.float32), sc.material_ids.astype(np.uint16), sc.object_ids.astype(np.uint32)
        rng = np.random.default_rng(0x5EC0)
        lo, hi = w.tri.reshape(-1, 3).min(axis=0), w.tri.reshape(-1, 3).max(axis=0)
        pos = rng.uniform(lo, hi, (64, 3)).astype(np.float32)
        lis = sc.listener
        _rooms.update(w=w, pos=pos, lis=lis, want=Restatement(oracle_mod, w).expect(pkg, pos, lis))
    return _rooms


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["sah", "device_morton"])
def test_rooms(pkg, oracle_mod, fast):
    rc = rooms_case(pkg, oracle_mod)
    assert len(rc["w"].tri) > 256, "one scan workgroup"
    ctx = rc["w"].context(pkg, fast=fast)
    ctx.set_listener(rc["lis"])
    h = place(ctx, rc["pos"])
    rows, paths = got = ctx.reflection_paths(h)
    assert_equal(got, rc["want"], f"rooms fast={fast}")
    assert len(set(rows["found"])) > 2 and np.any(rows["found"] < rows["candidates"])   # the case is not trivial
    contract.batch_agrees(ctx.reflection_paths, h, got, singles=not fast)
    ctx.close()


@pytest.mark.gpu
def test_mover(pkg, oracle_mod):
    # a door that stands in front of the x = 1000 wall's reflection point, then slides aside
    _, P = image_source(SRC, LIS, 1)
    door = box([900.0, P[1] - 100.0, 1.0], [910.0, P[1] + 100.0, 299.0])
    w = shoebox_world([(door, OPAQUE, 5)])
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, paths = check(pkg, ctx, Restatement(oracle_mod, w), h, [SRC], LIS, "door shut")
    shut = set(int(t) for t in paths[0]["triangle"][:rows[0]["returned"]])
    assert not shut & {2, 3} and any(t >= 12 for t in shut), "the wall behind the door reflects, or the door does not"
    aside = np.array([[1, 0, 0, 0], [0, 1, 0, -350], [0, 0, 1, 0]], np.float32)
    ctx.set_object_transforms([5], aside[None])
    rows, paths = check(pkg, ctx, Restatement(oracle_mod, w, contract.transformed(w, 5, aside)), h, [SRC], LIS, "door aside, no explicit refit")   # the call refits first
    opened = set(int(t) for t in paths[0]["triangle"][:rows[0]["returned"]])
    assert opened & {2, 3}, "the reflection the door uncovered did not appear"
    ctx.set_object_transforms([5], np.eye(3, 4, dtype=np.float32)[None])
    rows, paths = check(pkg, ctx, Restatement(oracle_mod, w), h, [SRC], LIS, "door back")
    assert set(int(t) for t in paths[0]["triangle"][:rows[0]["returned"]]) == shut
    ctx.close()


def _defaults_found(t, oracle_mod, want):
    assert tuple(want[0][0]) == (6, 6, 6, 0)


def _legal_found(rows):
    assert tuple(rows[0]) == (6, 0, 0, 1)


inf, nan = float("inf"), float("nan")
QUERY = contract.Query(
    kind="reflection", dtypes=("REFLECTION_ROW_DTYPE", "REFLECTION_DTYPE"), world=shoebox_world, src=SRC, lis=LIS, wrong_struct_size=32,
    refused=(dict(max_paths=0), dict(max_paths=17), dict(max_candidates=0), dict(max_candidates=257), dict(margin=-1e-3), dict(margin=nan),
             dict(margin=inf), dict(step=-0.1), dict(step=nan), dict(step=inf), dict(offset=-0.1), dict(offset=nan), dict(offset=inf),
             dict(pullback=-1.0), dict(pullback=nan), dict(pullback=inf), dict(dist_divisor=0.0), dict(dist_divisor=-1.0),
             dict(dist_divisor=nan), dict(dist_divisor=inf), dict(sound_speed=0.0), dict(sound_speed=-1.0), dict(sound_speed=nan),
             dict(sound_speed=inf)),
    defaults_found=_defaults_found, legal=(dict(max_paths=16, max_candidates=1, margin=0.0, step=0.0, offset=0.0, pullback=0.0),),
    legal_found=_legal_found, yardstick=Restatement, empty_world=lambda: World([], ALPHA, TAU, 4, SCAT),
    fewer=dict(max_paths=16))   # a smaller count, more paths: fits what is there


@pytest.mark.gpu
def test_errors_and_untouched_state(pkg, oracle_mod):
    contract.errors_and_untouched_state(pkg, oracle_mod, QUERY)


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    contract.steady_state_allocates_nothing(pkg, QUERY)


@pytest.mark.gpu
def test_component_layer(pkg, oracle_mod):
    """AudioRayTracingSubsystem.UpdateReflectionPaths is Context.reflection_paths over the active sources"""
    w = shoebox_world()
    sub = pkg.AudioRayTracingSubsystem(num_bands=4)
    sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
    sub.SetMaterials(w.absorption, w.transmission, w.scattering)
    positions = [SRC, [700.0, 100.0, 50.0]]
    comps = [pkg.FrequenSeeAudioComponent(p) for p in positions]
    for c in comps:
        c.OnRegister(sub)
    sub.SetListenerLocation(LIS)
    got = sub.UpdateReflectionPaths(max_paths=4)
    assert_equal(got, Restatement(oracle_mod, w).expect(pkg, positions, LIS, max_paths=4), "component layer")
    assert got[1].shape == (2, 4) and tuple(got[0][0]) == (6, 6, 4, 0)
    sub.Deinitialize()
