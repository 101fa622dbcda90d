"""fs_update_reflection2_paths: the second-order specular reflections of every source of a tick.

The yardstick is a Python restatement of include/frequensee.h's "second-order reflection paths" rule on numpy float32, built on the
first-order restatement of tests/test_reflection_paths.py (its exact fmaf, dot, cross, its leg and its brute-force closest hit): the
near test as array arithmetic over all triangles, the pair filter per b as array arithmetic over all near a, the three legs per
candidate as scalars.  Every field of every row and path must EQUAL it, floats by bit pattern.  The restatement itself is checked
without a GPU against the float64 image-source lattice of a shoebox whose reflection points are, by assertion, nowhere near a
triangle edge.
"""
import ctypes as C

import numpy as np
import pytest

pytest.register_assert_rewrite("path_query_contract")
import path_query_contract as contract  # noqa: E402
from path_query_contract import assert_equal  # noqa: E402
from test_reflection_paths import (ALPHA, BLOCKED, FREE, HI, LIS, LO, NO_MATERIAL, NO_OBJECT, OPAQUE, SCAT, SLAB, SRC, TARGET, TAU, WALLS, F,
                                   Restatement, World, bits, box, cross, dot, fmaf, margin64, place, shoebox_world)

DEFAULTS = dict(max_paths=16, max_near=16384, max_candidates=256, max_length=1500.0, margin=1e-3, step=0.1, offset=0.1, pullback=0.1,
                dist_divisor=1000.0, sound_speed=343.0)
OVERFLOW, NEAR_OVERFLOW = 1, 2
FAR = 1e6   # a max_length no path of the rooms reaches


class Reflection2(Restatement):
    def __init__(self, oracle_mod, w, tri=None):
        super().__init__(oracle_mod, w, tri)
        with np.errstate(all="ignore"):
            self.n = cross(self.e1, self.e2) if len(self.v0) else np.zeros((0, 3), np.float32)
            self.nn = dot(self.n, self.n) if len(self.v0) else np.zeros(0, np.float32)
        self.stats = dict(leg1_blocked=0, leg2_blocked=0, leg3_blocked=0, passed_own=0, side_passed=0, pairs=0)

    def near_set(self, S, L, own, max_length):
        """step 0 over all triangles at once: the input indices of the near triangles, ascending"""
        T = len(self.v0)
        if T == 0:
            return np.zeros(0, np.int64)
        with np.errstate(all="ignore"):
            a, b = S[None, :] - self.v0, L[None, :] - self.v0
            reach = np.maximum(np.sqrt(dot(self.e1, self.e1)), np.sqrt(dot(self.e2, self.e2)))
            inside = ((np.sqrt(dot(a, a)) + np.sqrt(dot(b, b))) - (reach + reach)) <= F(max_length)
        assert reach.dtype == np.float32
        is_own = np.array([int(o) != NO_OBJECT and int(o) in own for o in self.w.obj], bool) if own else np.zeros(T, bool)
        return np.nonzero((self.nn != 0) & ~is_own & inside)[0]

    @staticmethod
    def mt(o, D, v0, e1, e2, m):
        """MT(o, D, k) on float32 scalars: (passes, s)"""
        with np.errstate(all="ignore"):
            p = cross(D, e2)
            det = dot(e1, p)
            inv = F(1.0) / det
            tv = o - v0
            u = dot(tv, p) * inv
            q = cross(tv, e1)
            v = dot(D, q) * inv
            s = dot(e2, q) * inv
            return bool(det != 0 and u >= -m and v >= -m and (u + v) <= F(1.0) + m and s > 0 and s < 1), s

    def pairs(self, S, L, near, margin, max_length):
        """step 1: the ordered pairs (b, a) of near triangles that pass, as (a, b, D, S1) with input indices"""
        m, out = F(margin), []
        if len(near) < 2:
            return out
        with np.errstate(all="ignore"):
            v0, e1, e2, n, nn = self.v0[near], self.e1[near], self.e2[near], self.n[near], self.nn[near]
            tv = L[None, :] - v0
            hL = dot(tv, n)
            q = cross(tv, e1)
            e2q = dot(e2, q)
            for jb, b in enumerate(near):
                hS = dot(S - self.v0[b], self.n[b])
                if hS == 0:
                    continue
                k1 = (F(2.0) * hS) / self.nn[b]
                S1 = S - k1 * self.n[b]
                h1 = dot(S1[None, :] - v0, n)
                side = ((h1 > 0) & (hL > 0)) | ((h1 < 0) & (hL < 0))
                side[jb] = False
                self.stats["pairs"] += len(near) - 1
                self.stats["side_passed"] += int(side.sum())
                i = np.nonzero(side)[0]
                k2 = (F(2.0) * h1[i]) / nn[i]
                D = (S1[None, :] - k2[:, None] * n[i]) - L[None, :]
                p = cross(D, e2[i])
                det = dot(e1[i], p)
                inv = F(1.0) / det
                u = dot(tv[i], p) * inv
                v = dot(D, q[i]) * inv
                s = e2q[i] * inv
                ok = (det != 0) & (u >= -m) & (v >= -m) & ((u + v) <= F(1.0) + m) & (s > 0) & (s < 1) & (np.sqrt(dot(D, D)) <= F(max_length))
                assert D.dtype == np.float32 and s.dtype == np.float32
                for k in np.nonzero(ok)[0]:
                    Dk = D[k]
                    Q = np.array([fmaf(s[k], Dk[c], L[c]) for c in range(3)], np.float32)
                    hQ = dot(Q - self.v0[b], self.n[b])
                    if not ((hQ > 0 and hS > 0) or (hQ < 0 and hS < 0)):
                        continue
                    if self.mt(Q, S1 - Q, self.v0[b], self.e1[b], self.e2[b], m)[0]:
                        out.append((int(near[i[k]]), int(b), Dk.copy(), S1.copy()))
        return out

    def gains(self, tri):
        return self.reflectance(tri)

    def row(self, S, L, src_obj=NO_OBJECT, lis_obj=NO_OBJECT, **params):
        """(row dict, confirmed paths in the rule's order: all of them, not only max_paths)"""
        p = dict(DEFAULTS, **params)
        S32, L32 = np.array([F(x) for x in S], np.float32), np.array([F(x) for x in L], np.float32)
        own = {i for i in (src_obj, lis_obj) if i != NO_OBJECT}
        near = self.near_set(S32, L32, own, p["max_length"])
        if len(near) > p["max_near"]:
            return dict(near=len(near), candidates=0, found=0, returned=0, flags=NEAR_OVERFLOW), []
        cand = self.pairs(S32, L32, near, p["margin"], p["max_length"])
        if len(cand) > p["max_candidates"]:
            return dict(near=len(near), candidates=len(cand), found=0, returned=0, flags=OVERFLOW), []
        offset, paths = F(p["offset"]), []
        for a, b, D, S1 in cand:
            with np.errstate(all="ignore"):
                len1 = F(np.sqrt(dot(D, D)))
                inv = F(1.0) / len1
                d = [F(D[k] * inv) for k in range(3)]
            status, t1, PA = self.leg(list(L32), d, len1, own, a, p["step"])
            if status != TARGET:
                self.stats["leg1_blocked"] += 1
                continue
            E = np.array([F(S1[k] - PA[k]) for k in range(3)], np.float32)
            len2 = F(np.sqrt(dot(E, E)))
            if len2 == 0:
                continue
            inv2 = F(1.0) / len2
            d2 = [F(E[k] * inv2) for k in range(3)]
            status, tt, PB = self.leg([fmaf(offset, d2[k], PA[k]) for k in range(3)], d2, F(len2 - offset), own, b, p["step"])
            if status != TARGET:
                self.stats["leg2_blocked"] += 1
                continue
            t2 = F(offset + tt)
            e = np.array([F(S32[k] - PB[k]) for k in range(3)], np.float32)
            len3 = F(np.sqrt(dot(e, e)))
            if len3 == 0:
                continue
            inv3 = F(1.0) / len3
            d3 = [F(e[k] * inv3) for k in range(3)]
            status, _, _ = self.leg([fmaf(offset, d3[k], PB[k]) for k in range(3)], d3, F(F(len3 - offset) - F(p["pullback"])), own, -1, p["step"])
            if status != FREE:
                self.stats["leg3_blocked"] += 1
                continue
            length = F(F(t1 + t2) + len3)
            paths.append(dict(length=length, delay=F(F(length / F(p["dist_divisor"])) / F(p["sound_speed"])),
                              point=np.array([PA, PB], np.float32), direction=np.array(d, np.float32), triangle=np.array([a, b], np.uint32),
                              material=np.array([int(self.w.mat[a]), int(self.w.mat[b])], np.uint32),
                              reflectance=(self.gains(a) * self.gains(b)).astype(np.float32)))
        paths.sort(key=lambda x: (bits(x["length"]), int(x["triangle"][0]), int(x["triangle"][1])))
        return dict(near=len(near), candidates=len(cand), found=len(paths), returned=min(len(paths), p["max_paths"]), flags=0), paths

    def expect(self, pkg, positions, L, src_obj=None, lis_obj=NO_OBJECT, **params):
        """the call's two arrays as the library must write them"""
        mp = dict(DEFAULTS, **params)["max_paths"]
        rows = np.zeros(len(positions), dtype=pkg.Context.REFLECTION2_ROW_DTYPE)
        paths = np.zeros((len(positions), mp), dtype=pkg.Context.REFLECTION2_DTYPE)
        for i, S in enumerate(positions):
            r, ps = self.row(S, L, NO_OBJECT if src_obj is None else src_obj[i], lis_obj, **params)
            for k in rows.dtype.names:
                rows[i][k] = r[k]
            for j, x in enumerate(ps[:mp]):
                for k in paths.dtype.names:
                    paths[i, j][k] = x[k]
        return rows, paths


check = contract.checker("reflection2")


# ---- the float64 image-source lattice of the shoebox --------------------------------------------------------------------------
# SRC / LIS of the first-order tests, moved by a few tens of centimetres until the two preconditions of the lattice test hold at
# n = 1 and n = 4 (and at the n = 5 of the GPU case): 36 reflection points, none within 1.2e-2 of an edge on any of the meshes
SRC2, LIS2 = [SRC[0] - 38.0, SRC[1] - 2.0, SRC[2] - 18.0], [LIS[0] + 24.0, LIS[1] - 39.0, LIS[2] + 12.0]


def mirror(P, wall):
    axis, plane = wall // 2, (LO, HI)[wall % 2][wall // 2]
    M = np.array(P, np.float64)
    M[axis] = 2.0 * plane - M[axis]
    return M


def on_wall(P, wall, eps=1e-9):
    axis = wall // 2
    return all(LO[k] - eps <= P[k] <= HI[k] + eps for k in range(3) if k != axis)


def lattice(S, L):
    """float64: the second-order image paths of the room as (length, wall a, wall b, PA, PB), every ordered pair of distinct walls
    whose two reflection points lie on their walls in the order L -> PA -> PB -> S"""
    S, L, out = np.asarray(S, np.float64), np.asarray(L, np.float64), []
    for wb in range(6):
        S1 = mirror(S, wb)
        for wa in range(6):
            if wa == wb:
                continue
            S2 = mirror(S1, wa)
            axis, plane = wa // 2, (LO, HI)[wa % 2][wa // 2]
            if S2[axis] == L[axis]:
                continue
            s = (plane - L[axis]) / (S2[axis] - L[axis])
            PA = L + s * (S2 - L)
            if not (0.0 < s < 1.0 and on_wall(PA, wa)):
                continue
            axis, plane = wb // 2, (LO, HI)[wb % 2][wb // 2]
            if S1[axis] == PA[axis]:
                continue
            s = (plane - PA[axis]) / (S1[axis] - PA[axis])
            PB = PA + s * (S1 - PA)
            if not (0.0 < s < 1.0 and on_wall(PB, wb)):
                continue
            out.append((float(np.linalg.norm(S2 - L)), wa, wb, PA, PB))
    return sorted(out, key=lambda x: x[0])


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.Reflection2Params) == 44 and C.sizeof(cap.Reflection2Path) == 92 and C.sizeof(cap.Reflection2Row) == 20
    assert pkg.Context.REFLECTION2_DTYPE.itemsize == 92 and pkg.Context.REFLECTION2_ROW_DTYPE.itemsize == 20
    for (name, _), (dname) in zip(cap.Reflection2Path._fields_, pkg.Context.REFLECTION2_DTYPE.names):
        assert name == dname and getattr(cap.Reflection2Path, name).offset == pkg.Context.REFLECTION2_DTYPE.fields[name][1]
    p = cap.default_reflection2_params()
    assert p.struct_size == 44
    assert (p.max_paths, p.max_near, p.max_candidates) == (16, 16384, 256)
    assert p.max_length == 1500.0 and p.margin == F(1e-3) and p.step == F(0.1) and p.offset == F(0.1) and p.pullback == F(0.1)
    assert p.dist_divisor == 1000.0 and p.sound_speed == 343.0
    q = cap.default_reflection_params()
    assert all(getattr(p, k) == getattr(q, k) for k in ("margin", "step", "offset", "pullback", "dist_divisor", "sound_speed"))
    assert (cap.MAX_REFLECTION2_PATHS, cap.MAX_REFLECTION2_NEAR, cap.MAX_REFLECTION2_CANDIDATES, cap.MAX_REFLECTION2_BATCH) == (32, 32768, 1024, 256)
    assert cap.REFLECTION2_OVERFLOW != cap.REFLECTION2_NEAR_OVERFLOW and cap.REFLECTION2_OVERFLOW and cap.REFLECTION2_NEAR_OVERFLOW
    assert cap.load().fs_abi_version() == 5


def test_exported_in_one_tier(pkg):
    extended = contract.exported_in_one_tier(pkg, ("fs_reflection2_params_default", "fs_update_reflection2_paths"))
    assert "fs_update_reflection_paths" in extended.split()   # the tier of the first-order call


def test_null_context_and_no_device(pkg):
    contract.null_context_and_no_device(pkg, QUERY)


@pytest.mark.parametrize("n", [1, 4], ids=["12_triangles", "192_triangles"])
def test_restatement_against_image_lattice(pkg, oracle_mod, n):
    """S and L are chosen so that, in float64, every reflection point lies more than 1e-2 (barycentric) inside its triangle and no two
    lengths are closer than 1e-3 relative: eighteen paths — the images at lattice distance 2, one valid reflector order each — are a
    property of the input, not of rounding"""
    w = shoebox_world(n=n)
    per_wall = 2 * n * n
    want = lattice(SRC2, LIS2)
    assert len(want) == 18
    assert sorted((a // 2 == b // 2) for _, a, b, _, _ in want).count(True) == 6, "two per axis off opposite walls, twelve round a corner"
    assert len({tuple(np.round(mirror(mirror(SRC2, b), a), 6)) for _, a, b, _, _ in want}) == 18, "one reflector order per image"
    tris = []
    for _, wa, wb, PA, PB in want:
        for wall, P in ((wa, PA), (wb, PB)):
            m, tri = margin64(w.tri, P)
            assert m > 1e-2, f"wall {wall}: reflection point only {m} inside its triangle"
            assert tri // per_wall == wall
            tris.append(tri)
    lengths = [x[0] for x in want]
    assert all((b - a) / b > 1e-3 for a, b in zip(lengths, lengths[1:]))
    y = Reflection2(oracle_mod, w)
    r, paths = y.row(SRC2, LIS2, max_paths=32, max_length=FAR)
    assert r == dict(near=12 * n * n, candidates=18, found=18, returned=18, flags=0)
    assert [bits(p["length"]) for p in paths] == sorted(bits(p["length"]) for p in paths)
    size = float(np.max(np.asarray(HI) - np.asarray(LO)))
    for p, (ref, wa, wb, PA, PB), ta, tb in zip(paths, want, tris[0::2], tris[1::2]):
        # three legs of about twenty fp32 roundings of 6e-8 each: 1e-5 leaves nearly an order of magnitude
        assert abs(float(p["length"]) - ref) <= 1e-5 * ref, (wa, wb, p["length"], ref)
        assert (int(p["triangle"][0]), int(p["triangle"][1])) == (ta, tb)
        for wall, got, P in ((wa, p["point"][0], PA), (wb, p["point"][1], PB)):
            assert abs(float(got[wall // 2]) - (LO, HI)[wall % 2][wall // 2]) <= 1e-5 * size, (wall, got)
            assert np.allclose(got, P, rtol=0, atol=1e-5 * size * 10)
        g = y.spec[WALLS]
        assert np.array_equal(p["reflectance"][:4], g * g) and np.all(p["reflectance"][4:] == 0)
        assert np.all((p["reflectance"][:4] > 0) & (p["reflectance"][:4] < g))


def test_beyond_max_length_nothing_is_near(pkg, oracle_mod):
    """a listener and a source more than max_length apart — by more than twice the largest triangle's reach, which the bound allows
    every triangle — have no near triangle"""
    w = shoebox_world(n=8)
    y = Reflection2(oracle_mod, w)
    reach = float(np.hypot(1000.0 / 8, 800.0 / 8))
    assert float(np.linalg.norm(np.asarray(SRC) - np.asarray(LIS))) > 200.0 + 2.0 * reach * (1.0 + 1e-6)
    r, paths = y.row(SRC, LIS, max_length=200.0)
    assert r == dict(near=0, candidates=0, found=0, returned=0, flags=0) and not paths
    r, _ = y.row(SRC, LIS, max_length=400.0, max_candidates=1024)
    assert 0 < r["near"] < len(w.tri), "the bound is an ellipsoid: some triangles are near, some are not"


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5], ids=["12_triangles", "300_triangles"])
def test_shoebox(pkg, oracle_mod, n):
    """n = 1: fewer near triangles than one wave of a; n = 5: more than one workgroup of a and more than one LDS tile of b (both 256)"""
    w = shoebox_world(n=n)
    assert len(w.tri) == 12 * n * n
    ctx = w.context(pkg)
    ctx.set_listener(LIS2)
    rows, paths = check(pkg, ctx, Reflection2(oracle_mod, w), place(ctx, [SRC2]), [SRC2], LIS2, f"shoebox n={n}", max_paths=32, max_length=FAR)
    assert tuple(rows[0]) == (12 * n * n, 18, 18, 18, 0)
    assert np.all(paths[0][18:].view(np.uint8) == 0)
    ctx.close()


# ---- near lists that end at the edges of the pair kernel's tiles ---------------------------------------------------------
# The pair kernel streams a row's near list through LDS in tiles of 256 entries, shared among at most 16 workgroups per tile of a:
# a list of 255, 256 and 257 entries ends one entry either side of a tile's edge, one of 4100 has 17 tiles (one workgroup takes two).
TILE_EDGE_NEAR = (255, 256, 257, 4100)
_tile_edges = {}


def sparse_field(count):
    """count triangles of 1 cm, 12 cm apart under the ceiling: every one is near (max_length = FAR), the reflectors stay the walls"""
    k = np.arange(count)
    v0 = np.stack([60.0 + 12.0 * (k % 72), 40.0 + 12.0 * (k // 72), np.full(count, 285.0)], axis=1)
    return np.stack([v0, v0 + [1.0, 0.0, 0.0], v0 + [0.0, 1.0, 0.0]], axis=1).astype(np.float32)


def tile_edge_case(pkg, oracle_mod, near):
    """(world, the call's two arrays by the restatement) of the shoebox with near - 12 triangles of the sparse field — computed once"""
    if near not in _tile_edges:
        w = shoebox_world([(sparse_field(near - 12), OPAQUE, 3)])
        _tile_edges[near] = w, Reflection2(oracle_mod, w).expect(pkg, [SRC2], LIS2, max_paths=32, max_length=FAR)
    return _tile_edges[near]


@pytest.mark.parametrize("near", TILE_EDGE_NEAR)
def test_tile_edge_preconditions(pkg, oracle_mod, near):
    """the restatement alone: the near list has the length asked for, the candidates stay a handful and paths are found"""
    rows, paths = tile_edge_case(pkg, oracle_mod, near)[1]
    assert rows[0]["near"] == near and 0 < rows[0]["candidates"] <= 64 and rows[0]["returned"] > 0 and rows[0]["flags"] == 0
    assert np.all(paths[0]["length"][:rows[0]["returned"]] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("near", TILE_EDGE_NEAR)
def test_near_list_at_tile_edges(pkg, oracle_mod, near):
    w, want = tile_edge_case(pkg, oracle_mod, near)
    ctx = w.context(pkg)
    ctx.set_listener(LIS2)
    got = ctx.reflection2_paths(place(ctx, [SRC2]), max_paths=32, max_length=FAR)
    assert_equal(got, want, f"near list of {near}")
    assert got[0][0]["near"] == near and got[0][0]["returned"] > 0
    ctx.close()


@pytest.mark.gpu
def test_room_centre_equal_lengths(pkg, oracle_mod):
    """source and listener at the centre: the paths come in groups of one length, the rank within them is decided by (a, b)"""
    w = shoebox_world()
    ctx = w.context(pkg)
    centre = [500.0, 400.0, 150.0]
    ctx.set_listener(centre)
    rows, paths = check(pkg, ctx, Reflection2(oracle_mod, w), place(ctx, [centre]), [centre], centre, "centre", max_paths=32, max_length=FAR)
    got = paths[0][:rows[0]["returned"]]
    assert len(got) > 2 and len(set(got["length"].view(np.uint32).tolist())) < len(got), "no two paths of one length"
    ctx.close()


# source and listener above the diagonal (0, 0) - (1000, 800) that the floor's and the ceiling's two triangles share (y = 0.8 x, exact in
# fp32), at different heights: the xy projection of a floor-ceiling path is the straight segment between them, so PA and PB lie on it
EDGE_S, EDGE_L = [750.0, 600.0, 170.0], [250.0, 200.0, 110.0]
FLOOR, CEILING = 4, 5   # walls; their triangles at n = 1: 8, 9 and 10, 11


def shared_edge_case(oracle_mod):
    """(world, restatement) after the case's preconditions: in float64 the two floor-ceiling paths have both reflection points on the
    shared edge (barycentric margin 0 but for rounding), and in the restatement the pair filter passes, for either order of the two
    walls, all four combinations of their triangles — the case cannot slide off the edge unnoticed"""
    w = shoebox_world()
    on_edge = [x for x in lattice(EDGE_S, EDGE_L) if {x[1], x[2]} == {FLOOR, CEILING}]
    assert sorted((x[1], x[2]) for x in on_edge) == [(FLOOR, CEILING), (CEILING, FLOOR)]
    for _, wa, wb, PA, PB in on_edge:
        for wall, P in ((wa, PA), (wb, PB)):
            m, tri = margin64(w.tri, P)
            assert abs(m) < 1e-9 and tri // 2 == wall, (wall, P, m)
            assert abs(P[1] - 0.8 * P[0]) < 1e-9 and 0.0 < P[0] < 1000.0
    y = Reflection2(oracle_mod, w)
    S32, L32 = np.asarray(EDGE_S, np.float32), np.asarray(EDGE_L, np.float32)
    near = y.near_set(S32, L32, set(), FAR)
    assert len(near) == 12
    cand = {(a, b) for a, b, _, _ in y.pairs(S32, L32, near, DEFAULTS["margin"], FAR)}
    for ta, tb in ((8, 10), (8, 11), (9, 10), (9, 11)):
        assert (ta, tb) in cand and (tb, ta) in cand, (ta, tb, sorted(cand))
    return w, y


def test_shared_edge_preconditions(pkg, oracle_mod):
    shared_edge_case(oracle_mod)


@pytest.mark.gpu
def test_shared_edge_at_each_reflector(pkg, oracle_mod):
    """PA and PB of the floor-ceiling paths on the edge their wall's two triangles share (shared_edge_case asserts it).  Of the
    result only equality is asserted: either triangle, both or none may claim a point."""
    w, y = shared_edge_case(oracle_mod)
    ctx = w.context(pkg)
    ctx.set_listener(EDGE_L)
    rows, _ = check(pkg, ctx, y, place(ctx, [EDGE_S]), [EDGE_S], EDGE_L, "shared edge", max_paths=32, max_length=FAR)
    assert rows[0]["candidates"] >= 8
    ctx.close()


@pytest.mark.gpu
def test_no_and_one_near_triangle(pkg, oracle_mod):
    """triangles present and none or one of them near: the pair kernel's workgroups leave at once, the confirmation runs without
    a candidate"""
    # (the two triangles of a wall's cell share v0 and reach, so a wall alone never has one near triangle: a free-standing
    # triangle halfway between source and listener, of a larger reach than the walls' cells, is the one)
    lone = np.array([[[515.0, 395.0, 140.0], [665.0, 395.0, 140.0], [515.0, 495.0, 140.0]]], np.float32)
    w = shoebox_world([(lone, OPAQUE, 2)], n=8)
    y = Reflection2(oracle_mod, w)
    S32, L32 = np.asarray(SRC, np.float32), np.asarray(LIS, np.float32)
    a, b = S32[None, :] - y.v0, L32[None, :] - y.v0
    reach = np.maximum(np.sqrt(dot(y.e1, y.e1)), np.sqrt(dot(y.e2, y.e2)))
    bound = np.sort((np.sqrt(dot(a, a)) + np.sqrt(dot(b, b))) - (reach + reach))
    assert bound.dtype == np.float32 and 200.0 < bound[0] < bound[1]
    one = float(bound[0]) + 0.5 * (float(bound[1]) - float(bound[0]))
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC, SRC])
    rows, paths = check(pkg, ctx, y, h, [SRC, SRC], LIS, "no near triangle", max_length=200.0)
    assert all(tuple(r) == (0, 0, 0, 0, 0) for r in rows) and np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC, SRC], LIS, "one near triangle", max_length=one)
    assert all(tuple(r) == (1, 0, 0, 0, 0) for r in rows) and np.all(paths.view(np.uint8) == 0)
    ctx.close()


@pytest.mark.gpu
def test_blocked_legs(pkg, oracle_mod):
    """a partition across most of the room between source and listener and a half wall beside the listener: each of the three legs
    is blocked for some candidate of some source"""
    w = shoebox_world([(box([495.0, 1.0, 1.0], [505.0, 600.0, 299.0]), SLAB, 2), (box([600.0, 300.0, 1.0], [610.0, 799.0, 200.0]), OPAQUE, 2)])
    y = Reflection2(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    pos = [SRC, [120.0, 650.0, 60.0], [400.0, 330.0, 222.0], [650.0, 700.0, 250.0], [560.0, 100.0, 40.0], [650.0, 300.0, 150.0]]
    rows, paths = check(pkg, ctx, y, place(ctx, pos), pos, LIS, "blocked legs", max_paths=32, max_length=FAR)
    assert y.stats["leg1_blocked"] > 0 and y.stats["leg2_blocked"] > 0 and y.stats["leg3_blocked"] > 0, y.stats
    assert len(set(rows["found"])) > 1 and np.any(rows["found"] < rows["candidates"])
    assert np.any(paths["triangle"] >= 12), "no reflection off the partitions"
    ctx.close()


@pytest.mark.gpu
def test_coplanar_pair_yields_nothing(pkg, oracle_mod):
    """a single wall cut into 32 triangles: every pair is coplanar, S1 lies behind the plane the listener is in front of"""
    from test_reflection_paths import quad_grid
    wall = np.asarray(quad_grid([0.0, 0.0, 0.0], [1000.0, 0.0, 0.0], [0.0, 800.0, 0.0], 4), np.float32)
    w = World([(wall, WALLS, 1)], ALPHA, TAU, 4, SCAT)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Reflection2(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, "coplanar", max_length=FAR)
    assert tuple(rows[0]) == (32, 0, 0, 0, 0) and np.all(paths.view(np.uint8) == 0)
    assert ctx.reflection_paths(place(ctx, [SRC]))[0][0]["found"] == 1, "the wall does reflect once"
    ctx.close()


@pytest.mark.gpu
def test_own_actors(pkg, oracle_mod):
    s, l = np.asarray(SRC2), np.asarray(LIS2)
    w = shoebox_world([(box(s - 25.0, s + 25.0), OPAQUE, 8), (box(l - 30.0, l + 30.0), OPAQUE, 7)])
    y = Reflection2(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS2)
    h = place(ctx, [SRC2])
    # foreign ids: the two meshes block every leg (both ends are boxed in) and reflect what starts inside them
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "foreign meshes", max_paths=32, max_length=FAR)
    assert rows[0]["near"] == 36
    assert not np.any(paths[0]["triangle"][:rows[0]["returned"]] < 12), "a wall was reached through a closed box"
    ctx.set_source_object(h[0], 8)
    ctx.set_listener_object(7)
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "own meshes", src_obj=[8], lis_obj=7, max_paths=32, max_length=FAR)
    assert y.stats["passed_own"] > 0
    assert tuple(rows[0]) == (12, 18, 18, 18, 0) and np.all(paths[0]["triangle"][:18] < 12), "an own mesh reflected, blocked or was near"
    ctx.close()


@pytest.mark.gpu
def test_caps(pkg, oracle_mod):
    w = shoebox_world()
    y = Reflection2(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS2)
    h = place(ctx, [SRC2])
    full = ctx.reflection2_paths(h, max_paths=32, max_length=FAR)
    assert tuple(full[0][0]) == (12, 18, 18, 18, 0)
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "near exactly at the cap", max_near=12, max_paths=32, max_length=FAR)
    assert rows.tobytes() == full[0].tobytes() and paths.tobytes() == full[1].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "near overflow", max_near=11, max_paths=32, max_length=FAR)
    assert tuple(rows[0]) == (12, 0, 0, 0, pkg._capi.REFLECTION2_NEAR_OVERFLOW) and np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "candidates exactly at the cap", max_candidates=18, max_paths=32, max_length=FAR)
    assert rows.tobytes() == full[0].tobytes() and paths.tobytes() == full[1].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "candidate overflow", max_candidates=17, max_paths=32, max_length=FAR)
    assert tuple(rows[0]) == (12, 18, 0, 0, pkg._capi.REFLECTION2_OVERFLOW) and np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "five shortest", max_paths=5, max_length=FAR)
    assert tuple(rows[0]) == (12, 18, 18, 5, 0) and paths.shape == (1, 5) and paths[0].tobytes() == full[1][0][:5].tobytes()
    # max_length just above and just below the seventh path's length: the path is in, then out (and with it every longer one)
    seventh = full[1][0][6]["length"]
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "length cap above", max_paths=32, max_length=float(seventh) * (1.0 + 1e-5))
    assert rows[0]["found"] == 7 and paths[0][:7].tobytes() == full[1][0][:7].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC2], LIS2, "length cap below", max_paths=32, max_length=float(seventh) * (1.0 - 1e-5))
    assert rows[0]["found"] == 6 and paths[0][:6].tobytes() == full[1][0][:6].tobytes()
    ctx.close()


@pytest.mark.gpu
def test_materials_and_degenerate_triangles(pkg, oracle_mod):
    room = box(LO, HI)
    degenerate = np.array([[[0.0, 100.0, 100.0], [0.0, 100.0, 100.0], [0.0, 300.0, 200.0]],      # two corners equal
                           [[100.0, 0.0, 50.0], [300.0, 0.0, 150.0], [500.0, 0.0, 250.0]],       # three on a line
                           [[400.0, 300.0, 0.0], [400.0, 300.0, 0.0], [400.0, 300.0, 0.0]]], np.float32)   # a point
    # walls x: material 0; walls y: no material; walls z: an id beyond the table; three bands
    w = World([(room[0:4], 0, 1), (room[4:8], NO_MATERIAL, 1), (room[8:12], 9, 1), (degenerate, 0, 1)], [a[:3] for a in ALPHA], [t[:3] for t in TAU], 3, [x[:3] for x in SCAT])
    y = Reflection2(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS2)
    rows, paths = check(pkg, ctx, y, place(ctx, [SRC2]), [SRC2], LIS2, "materials", max_paths=32, max_length=FAR)
    assert tuple(rows[0]) == (12, 18, 18, 18, 0), "a degenerate triangle was near"
    g, kinds = y.spec[0], set()
    for p in paths[0][:18]:
        with_material = [int(m) == 0 for m in p["material"]]
        assert all(int(p["material"][k]) == w.mat[p["triangle"][k]] for k in range(2)) and np.all(p["reflectance"][3:] == 0)
        want = np.ones(3, np.float32)
        for k in range(2):
            want = want * (g if with_material[k] else np.ones(3, np.float32))
        assert np.array_equal(p["reflectance"][:3], want)
        kinds.add(sum(with_material))
    assert kinds == {0, 1, 2}, "no path with none, one and two surfaces of the material"
    for k in ("length", "delay", "point", "direction", "reflectance"):
        assert np.all(np.isfinite(paths[k]))
    ctx.close()


_rooms = {}


def rooms_case(pkg, oracle_mod):
    """starter_room with synthetic lobes, the first 8 of the 64 seeded sources of the first-order tests, and the restatement's arrays —
    computed once"""
    if not _rooms:
        sc = pkg.scenes.starter_room(4)
        tr, sca = pkg.scenes.material_lobes(sc)
        w = World([], sc.absorption, tr, 4, sca)
        w.tri, w.mat, w.obj = sc.triangles.astype(np.float32), sc.material_ids.astype(np.uint16), sc.object_ids.astype(np.uint32)
        rng = np.random.default_rng(0x5EC0)
        lo, hi = w.tri.reshape(-1, 3).min(axis=0), w.tri.reshape(-1, 3).max(axis=0)
        pos = rng.uniform(lo, hi, (64, 3)).astype(np.float32)[:8]
        lis = sc.listener
        _rooms.update(w=w, pos=pos, lis=lis, want=Reflection2(oracle_mod, w).expect(pkg, pos, lis, max_length=FAR))
    return _rooms


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["sah", "device_morton"])
def test_rooms(pkg, oracle_mod, fast):
    rc = rooms_case(pkg, oracle_mod)
    wrows = rc["want"][0]
    assert not np.any(wrows["flags"]) and len(set(wrows["found"])) > 1 and np.all(wrows["near"] > 256)   # the case is not trivial
    ctx = rc["w"].context(pkg, fast=fast)
    ctx.set_listener(rc["lis"])
    h = place(ctx, rc["pos"])
    rows, paths = got = ctx.reflection2_paths(h, max_length=FAR)
    assert_equal(got, rc["want"], f"rooms fast={fast}")
    contract.batch_agrees(ctx.reflection2_paths, h, got, singles=not fast, max_length=FAR)
    ctx.close()


@pytest.mark.gpu
def test_mover(pkg, oracle_mod):
    """a door that stands in front of the x = 1000 wall, then slides aside: the call refits first"""
    door = box([900.0, 300.0, 1.0], [910.0, 700.0, 299.0])
    w = shoebox_world([(door, OPAQUE, 5)])
    ctx = w.context(pkg)
    ctx.set_listener(LIS2)
    h = place(ctx, [SRC2])
    rows, paths = check(pkg, ctx, Reflection2(oracle_mod, w), h, [SRC2], LIS2, "door shut", max_paths=32, max_length=FAR)
    shut = paths[0][:rows[0]["returned"]].copy()
    assert np.any(shut["triangle"] >= 12), "the door does not reflect"
    aside = np.array([[1, 0, 0, 0], [0, 1, 0, -290], [0, 0, 1, 0]], np.float32)
    ctx.set_object_transforms([5], aside[None])
    rows, paths = check(pkg, ctx, Reflection2(oracle_mod, w, contract.transformed(w, 5, aside)), h, [SRC2], LIS2, "door aside, no explicit refit", max_paths=32, max_length=FAR)
    assert paths[0][:rows[0]["returned"]].tobytes() != shut.tobytes(), "the door moved and nothing changed"
    ctx.set_object_transforms([5], np.eye(3, 4, dtype=np.float32)[None])
    rows, paths = check(pkg, ctx, Reflection2(oracle_mod, w), h, [SRC2], LIS2, "door back", max_paths=32, max_length=FAR)
    assert paths[0][:rows[0]["returned"]].tobytes() == shut.tobytes()
    ctx.close()


def _defaults_found(t, oracle_mod, want):
    """the defaults' max_length leaves some of the 18 paths out"""
    assert_equal(want, Reflection2(oracle_mod, t.w).expect(t.pkg, [SRC2, SRC2], LIS2), "defaults, one handle twice")
    assert 0 < want[0][0]["found"] < 18 and want[0][0]["flags"] == 0


def _legal_found(rows):
    assert tuple(rows[0]) == (12, 18, 0, 0, 1)


def _steady_found(ctx, h, first, fewer):
    assert np.all(first[0]["found"] == 18) and np.all(first[0]["returned"] == 16) and np.all(fewer[0]["returned"] == 18)


inf, nan = float("inf"), float("nan")
QUERY = contract.Query(
    kind="reflection2", dtypes=("REFLECTION2_ROW_DTYPE", "REFLECTION2_DTYPE"), world=shoebox_world, src=SRC2, lis=LIS2, wrong_struct_size=36,
    sentinel_paths=32, null_paths=16, refused_without_device=(dict(max_length=0.0),),
    refused=(dict(max_paths=0), dict(max_paths=33), dict(max_near=0), dict(max_near=32769), dict(max_candidates=0), dict(max_candidates=1025),
             dict(max_length=0.0), dict(max_length=-1.0), dict(max_length=nan), dict(max_length=inf), dict(margin=-1e-3), dict(margin=nan),
             dict(margin=inf), dict(step=-0.1), dict(step=nan), dict(step=inf), dict(offset=-0.1), dict(offset=nan), dict(offset=inf),
             dict(pullback=-1.0), dict(pullback=nan), dict(pullback=inf), dict(dist_divisor=0.0), dict(dist_divisor=-1.0),
             dict(dist_divisor=nan), dict(dist_divisor=inf), dict(sound_speed=0.0), dict(sound_speed=-1.0), dict(sound_speed=nan),
             dict(sound_speed=inf)),
    defaults_found=_defaults_found,
    legal=(dict(max_paths=32, max_near=32768, max_candidates=1, max_length=1e30, margin=0.0, step=0.0, offset=0.0, pullback=0.0),),
    legal_found=_legal_found, yardstick=Reflection2, empty_world=lambda: World([], ALPHA, TAU, 4, SCAT),
    steady=dict(max_length=FAR), fewer=dict(max_paths=32, max_near=32768, max_candidates=1024), fewer_differs_in=("returned",),
    steady_found=_steady_found)


@pytest.mark.gpu
def test_errors_and_untouched_state(pkg, oracle_mod):
    contract.errors_and_untouched_state(pkg, oracle_mod, QUERY)


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    contract.steady_state_allocates_nothing(pkg, QUERY)


@pytest.mark.gpu
def test_queries_interleaved_on_one_context(pkg):
    """the four queries share their chain, scan and staging code but no buffer: on one context, in an order in which every staging is
    used, grown past its first capacity of 32 (count 33) and used again with fewer rows, each call returns the bytes it returns as the
    first call of a fresh context"""
    from test_diffraction_paths import interleaved_positions, sheet_world
    w = sheet_world(4)
    pos = interleaved_positions()

    def fresh():
        ctx = w.context(pkg)
        ctx.set_listener(LIS)
        return ctx, place(ctx, pos)

    calls = [("reflection2", 5), ("diffraction", 5), ("direct", 33), ("reflection", 1), ("reflection2", 33), ("diffraction", 33), ("reflection", 33),
             ("reflection2", 1), ("direct", 5), ("reflection", 5), ("reflection2", 5), ("diffraction", 1)]
    got = contract.queries_interleaved_on_one_context(fresh, calls, dict(reflection2=dict(max_length=FAR)))
    # the comparison is not of zeros
    assert np.any(got[4][0]["returned"] > 0) and np.any(got[5][0]["returned"] > 0) and np.any(got[6][0]["returned"] > 0)
    assert got[0][0].tobytes() == got[10][0].tobytes() and got[0][1].tobytes() == got[10][1].tobytes()


@pytest.mark.gpu
def test_component_layer(pkg, oracle_mod, monkeypatch):
    """UpdateReflection2Paths is Context.reflection2_paths over the active sources; Voices(second=) appends one voice per second-order
    path under keys no other path kind has, the callback they appear in reports all listed voices as started; of two paths whose
    keys collide the longer is dropped"""
    from test_direct_render import noise
    w = shoebox_world()
    frame, taps = 64, 15
    sub = pkg.AudioRayTracingSubsystem(num_bands=4)
    sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
    sub.SetMaterials(w.absorption, w.transmission, w.scattering)
    comp = pkg.FrequenSeeAudioComponent(SRC2)
    comp.OnRegister(sub)
    sub.SetListenerLocation(LIS2)
    plug = pkg.FrequenSeeAudioReflectionPlugin(sub)
    plug.Initialize(frame, taps, 32, 0.05)
    plug.OnInitSource(comp)
    rows, paths = sub.UpdateReflectionPaths(max_paths=8)
    srows, spaths = got = sub.UpdateReflection2Paths(max_paths=18, max_length=FAR)
    assert_equal(got, Reflection2(oracle_mod, w).expect(pkg, [SRC2], LIS2, max_paths=18, max_length=FAR), "component layer")
    voices = plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0], second=(srows[0], spaths[0]))
    nr, ns = int(rows[0]["returned"]), int(srows[0]["returned"])
    assert (nr, ns) == (6, 18)
    # h >> 2 drops the low bits of b: paths off one a and two b of one group of four share a key, and the earlier of the row stays
    keys = [0x40000000 | (((int(p["triangle"][0]) * 2654435761 + int(p["triangle"][1])) % 2 ** 32) >> 2) for p in spaths[0]]
    stay = [i for i, k in enumerate(keys) if k not in keys[:i]]
    assert voices.shape == (nr + len(stay),) and len(stay) >= 12
    assert np.array_equal(voices[:nr], plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0])), "the reflections' voices changed"
    latency = ((taps - 1) // 2) / sub.ctx.cfg.sample_rate
    for v, i in zip(voices[nr:], stay):
        p = spaths[0][i]
        assert int(v["key"]) == keys[i] == plug.SecondOrderKey(p["triangle"][0], p["triangle"][1])
        assert 0x40000000 <= int(v["key"]) < 0x80000000
        assert np.array_equal(v["band_gain"], p["reflectance"])
        assert float(v["delay"]) == pytest.approx(float(p["delay"]) - latency, abs=1e-7)
    listed = len(voices)
    assert len(set(voices["key"].tolist())) == listed
    rng = np.random.default_rng(5)
    out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, right=[0.0, 1.0, 0.0], second=(srows, spaths))
    assert int(counts[0]["started"]) == listed and int(counts[0]["dropped"]) == 0
    out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, right=[0.0, 1.0, 0.0], second=(srows, spaths))
    assert int(counts[0]["started"]) == 0 and int(counts[0]["sounding"]) == listed, "a steady source starts nothing"
    # a forced collision: every second-order path under one key — the first of the row, the shortest, is the one that stays
    monkeypatch.setattr(type(plug), "SecondOrderKey", staticmethod(lambda a, b: 0x40000000 | 5))
    collided = plug.Voices(rows[0], paths[0], second=(srows[0], spaths[0]))
    assert collided.shape == (nr + 1,) and int(collided[nr]["key"]) == 0x40000005
    assert np.array_equal(collided[nr]["band_gain"], spaths[0][0]["reflectance"])
    assert float(collided[nr]["delay"]) == pytest.approx(float(spaths[0][0]["delay"]) - latency, abs=1e-7)
    assert spaths[0][0]["length"] < spaths[0][1]["length"]
    out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, second=(srows, spaths))
    assert int(counts[0]["dropped"]) == 0, "the renderer was handed duplicate keys"
    plug.OnReleaseSource(comp)
    sub.Deinitialize()
