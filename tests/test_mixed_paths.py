"""fs_update_mixed_paths: the paths of every source of a tick that reflect off one triangle and bend round one edge.

The yardstick is a Python restatement of include/frequensee.h's "mixed paths" rule on numpy float32, built on the restatements of
tests/test_diffraction2_paths.py (its edge records, its construction at an apex, its legs), tests/test_diffraction_paths.py (the
exact fmaf on arrays) and tests/test_reflection_paths.py (the leg that asks for one triangle, the specular gain): the near sets as
array arithmetic, the filter per (face, end) as array arithmetic over all near edge records, the four legs per candidate as scalars
round the oracle's brute-force closest hit.  Every field of every row and path must EQUAL it, floats by bit pattern.  The restatement
itself is checked without a GPU against an independent float64 model: mirror the end next to the reflector in the reflector's plane,
unfold the two half-planes that meet in the rim about its line, intersect the unfolded segment with the reflector's plane, and keep
what the partition does not cut.

The scene is the issue's: a 1000 cm cube, a thin partition at x = 500 over y = 0 .. 600 from floor to ceiling with one free
vertical rim at y = 600, S = (250, 200, 150), L = (750, 200, 150).  Two things about it are facts of its geometry, found while the
float64 model was written, and the tests state them instead of what the issue expected:
  * S and L are mirror images of each other in the partition's plane, at one height.  The floor bounce's unfolded segment then meets
    the rim's line exactly at the floor (z = 0) and the ceiling bounce's exactly at the ceiling: R = E, the foot and the head of the
    rim, s = 0 in the plane intersection.  That degenerate limit is no path for the model or the rule, so this S and L have four
    paths (the walls x = 0, x = 1000 and, for either end, y = 0), not eight.  The floor and the ceiling are covered by a second
    listener, LIS2, off that symmetry.
  * All four paths bend at one apex, (500, 600, 150), so the legs at the apex are shared: the two paths of one end have the same leg
    from the rim to that end, and all four the same short leg.  A blocker across such a leg removes every path that runs through
    it; the blocker tests assert exactly that set, one path for the two legs at the reflector.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytest.register_assert_rewrite("path_query_contract")
import path_query_contract as contract  # noqa: E402
from path_query_contract import assert_equal  # noqa: E402
from test_diffraction_paths import fmaf_arrays
from test_diffraction2_paths import Diffraction2
from test_reflection_paths import (ALPHA, FREE, NO_MATERIAL, NO_OBJECT, OPAQUE, SCAT, TARGET, TAU, WALLS, F, World, bits, box, cross,
                                   dot, fmaf, place, quad_grid)

DEFAULTS = dict(max_paths=8, max_near=16384, max_candidates=1024, max_length=500.0, max_detour=1000.0, margin=1e-3, offset=0.1, merge=1.0,
                step=0.1, pullback=0.1, dist_divisor=1000.0, sound_speed=343.0)
OVERFLOW, NEAR_OVERFLOW = 1, 2
TAG = 0xC0000000
REACH = dict(max_length=2000.0)   # what the scene's tests ask for: its paths are 1310 to 1500 cm long, the default looks 500 cm far


def voice_key(p):
    return TAG | (((int(p["triangle"][0]) * 2654435761 + 4 * (2 * (4 * int(p["triangle"][1]) + int(p["edge"])) + int(p["end"]))) % 2 ** 32) >> 2)


class Mixed(Diffraction2):
    """edge record r = 3 i + j as in Diffraction2; a face is its triangle's input index"""

    def __init__(self, oracle_mod, w, tri=None, edges=None):
        super().__init__(oracle_mod, w, tri, edges)
        self.mx = dict(blocked=[0, 0, 0, 0], merged=0)

    def near_sets(self, S, L, own, max_length):
        """step 0: (the near faces, the near edge records), each ascending"""
        if len(self.v0) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        is_own = np.array([int(o) != NO_OBJECT and int(o) in own for o in self.w.obj], bool) if own else np.zeros(len(self.v0), bool)
        with np.errstate(all="ignore"):
            a, b = S[None, :] - self.v0, L[None, :] - self.v0
            reach = np.maximum(np.sqrt(dot(self.e1, self.e1)), np.sqrt(dot(self.e2, self.e2)))
            face = ((np.sqrt(dot(a, a)) + np.sqrt(dot(b, b))) - (reach + reach)) <= F(max_length)
            rS, rL = S[None, :] - self.ra, L[None, :] - self.ra
            er = np.sqrt(self.rww)
            edge = ((np.sqrt(dot(rS, rS)) + np.sqrt(dot(rL, rL))) - (er + er)) <= F(max_length)
        assert reach.dtype == np.float32 and er.dtype == np.float32
        faces = np.nonzero((self.rnn[::3] != 0) & ~is_own & face)[0]
        edges = np.nonzero((self.rnn != 0) & (self.rww != 0) & (self.roo != 0) & ~np.repeat(is_own, 3) & edge)[0]
        return faces, edges

    def triples(self, S, L, faces, edges, p):
        """step 1: the (m, r, end) that pass, each with the values the legs and the row use"""
        out = []
        if len(faces) == 0 or len(edges) == 0:
            return out
        mg, md, ml, one = F(p["margin"]), F(p["max_detour"]), F(p["max_length"]), F(1.0)
        a, w, ww, n, v0, o = self.ra[edges], self.rw[edges], self.rww[edges], self.rn[edges], self.rv0[edges], self.ro[edges]
        with np.errstate(all="ignore"):
            for m in faces:
                nm, nnm, v0m, e1m, e2m = self.rn[3 * m], self.rnn[3 * m], self.v0[m], self.e1[m][None, :], self.e2[m][None, :]
                for end in (0, 1):
                    A = S if end else L
                    hA = dot(A - v0m, nm)
                    if hA == 0:
                        continue
                    k = (F(2.0) * hA) / nnm
                    A1 = A - k * nm
                    assert A1.dtype == np.float32
                    Ss, Ls = (A1, L) if end else (S, A1)
                    hS, hL = dot(Ss[None, :] - v0, n), dot(Ls[None, :] - v0, n)
                    ok = (edges // 3 != m) & (((hS > 0) & (hL < 0)) | ((hS < 0) & (hL > 0)))
                    if not ok.any():
                        continue
                    rS, rL = Ss[None, :] - a, Ls[None, :] - a
                    tS, tL = dot(rS, w) / ww, dot(rL, w) / ww
                    cS, cL = cross(rS, w), cross(rL, w)
                    dS, dL = np.sqrt(dot(cS, cS) / ww), np.sqrt(dot(cL, cL) / ww)
                    total = dS + dL
                    t = tS + ((tL - tS) * dS) / total
                    ok &= (total != 0) & (t >= -mg) & (t <= one + mg)
                    E = fmaf_arrays(t[:, None], w, a)
                    u, v = Ss[None, :] - E, E - Ls[None, :]
                    lS, lL = np.sqrt(dot(u, u)), np.sqrt(dot(v, v))
                    length = lS + lL
                    g = Ss - Ls
                    bend = length - np.sqrt(dot(g, g))
                    s = hS / (hS - hL)
                    X = fmaf_arrays(s[:, None], (Ls - Ss)[None, :], Ss[None, :])
                    ok &= (lS != 0) & (lL != 0) & (bend <= md) & (length <= ml) & (dot(X - E, o) <= 0)
                    D = A1[None, :] - E
                    pv = cross(D, e2m)
                    det = dot(e1m, pv)
                    inv = one / det
                    tv = E - v0m[None, :]
                    bu = dot(tv, pv) * inv
                    q = cross(tv, e1m)
                    bv = dot(D, q) * inv
                    bs = dot(e2m, q) * inv
                    ok &= (det != 0) & (bu >= -mg) & (bv >= -mg) & ((bu + bv) <= one + mg) & (bs > 0) & (bs < 1)
                    for x in (E, length, bend, bu, bs):
                        assert x.dtype == np.float32
                    for i in np.nonzero(ok)[0]:
                        out.append(dict(m=int(m), r=int(edges[i]), end=end, E=E[i].copy(), A1=A1.copy(), u=u[i].copy(), v=v[i].copy(), lS=lS[i],
                                        lL=lL[i], length=length[i], bend=bend[i], hZ=(hL if end else hS)[i], t=t[i]))
        return out

    def legs(self, S32, L32, own, c, p, stop_at_first=True):
        """step 2 for candidate c: ({leg: reached or hit}, R, d4), the short leg first; the verdicts of legs 1 and 2 are independent,
        leg 4 exists only behind leg 3"""
        off, pb, step = F(p["offset"]), F(p["pullback"]), p["step"]
        A, Z = (S32, L32) if c["end"] else (L32, S32)
        nh, EZ, EA = self.ends(c["r"], c["hZ"], c["E"], off)
        verdict, R, d4 = {}, None, None
        verdict[2] = self.reached(EZ, [-x for x in nh], F(F(2.0) * off), own, step)
        if stop_at_first and not verdict[2]:
            return verdict, R, d4
        verdict[1] = self.long_leg(EZ, Z, pb, own, step)
        if stop_at_first and not verdict[1]:
            return verdict, R, d4
        e = np.array([F(c["A1"][k] - EA[k]) for k in range(3)], np.float32)
        ln3 = F(np.sqrt(dot(e, e)))
        with np.errstate(all="ignore"):
            inv = F(1.0) / ln3
            d = [F(e[k] * inv) for k in range(3)]
        status, _, R = self.leg(EA, d, ln3, own, c["m"], step)
        verdict[3] = status == TARGET
        if not verdict[3]:
            return verdict, None, d4
        e = np.array([F(A[k] - R[k]) for k in range(3)], np.float32)
        ln4 = F(np.sqrt(dot(e, e)))
        if ln4 == 0:
            verdict[4] = False
            return verdict, R, d4
        inv = F(1.0) / ln4
        d4 = [F(e[k] * inv) for k in range(3)]
        o4 = [fmaf(off, d4[k], R[k]) for k in range(3)]
        verdict[4] = self.leg(o4, d4, F(F(ln4 - off) - pb), own, -1, step)[0] == FREE
        return verdict, R, d4

    def row(self, S, L, src_obj=NO_OBJECT, lis_obj=NO_OBJECT, **params):
        """(row dict, the kept paths in the rule's order: all of them, not only max_paths)"""
        p = dict(DEFAULTS, **params)
        S32, L32 = np.array([F(c) for c in S], np.float32), np.array([F(c) for c in L], np.float32)
        own = {i for i in (src_obj, lis_obj) if i != NO_OBJECT}
        zero = dict(near=0, candidates=0, confirmed=0, found=0, returned=0, flags=0)
        faces, edges = self.near_sets(S32, L32, own, p["max_length"])
        near = len(faces) + len(edges)
        if near > p["max_near"]:
            return dict(zero, near=near, flags=NEAR_OVERFLOW), []
        cand = self.triples(S32, L32, faces, edges, p)
        if len(cand) > p["max_candidates"]:
            return dict(zero, near=near, candidates=len(cand), flags=OVERFLOW), []
        conf = []
        for c in cand:
            verdict, R, d4 = self.legs(list(S32), list(L32), own, c, p)
            if all(verdict.get(k, False) for k in (1, 2, 3, 4)):
                conf.append(dict(c, R=np.array(R, np.float32), d4=np.array(d4, np.float32),
                                 key=(bits(c["length"]), c["end"], c["m"], self.code(c["r"]))))
            else:
                self.mx["blocked"][[k for k in (2, 1, 3, 4) if not verdict.get(k, False)][0] - 1] += 1
        mm = F(p["merge"]) * F(p["merge"])
        kept = []
        for c in conf:
            if any(d["key"] < c["key"] and d["end"] == c["end"] and d["m"] == c["m"] and dot(c["E"] - d["E"], c["E"] - d["E"]) < mm for d in conf):
                self.mx["merged"] += 1
            else:
                kept.append(c)
        kept.sort(key=lambda c: c["key"])
        g = S32 - L32
        distance = np.sqrt(dot(g, g))
        ss, dd = float(F(p["sound_speed"])), float(F(p["dist_divisor"]))
        paths = []
        for c in kept:
            gm = self.reflectance(c["m"])
            gain = np.zeros(8, np.float32)
            for b in range(self.B):
                k = F(40.0 * self.f[b] / (ss * dd))
                gain[b] = gm[b] * (F(1.0) / np.sqrt(F(3.0) + k * c["bend"]))
            i = c["r"] // 3
            direction = c["v"] * (F(1.0) / c["lL"]) if c["end"] else -c["d4"]
            paths.append(dict(length=c["length"], delay=F(F(c["length"] / F(p["dist_divisor"])) / F(p["sound_speed"])),
                              detour=c["length"] - distance, bend_detour=c["bend"], cos_bend=dot(c["u"], c["v"]) / (c["lS"] * c["lL"]),
                              apex=c["E"], point=c["R"], direction=direction, end=c["end"], triangle=np.array([c["m"], i], np.uint32),
                              edge=c["r"] % 3, material=np.array([int(self.w.mat[c["m"]]), int(self.w.mat[i])], np.uint32), gain=gain, t=c["t"]))
        return dict(near=near, candidates=len(cand), confirmed=len(conf), found=len(kept), returned=min(len(kept), p["max_paths"]), flags=0), paths

    def expect(self, pkg, positions, L, src_obj=None, lis_obj=NO_OBJECT, **params):
        """the call's two arrays as the library must write them"""
        mp = dict(DEFAULTS, **params)["max_paths"]
        rows = np.zeros(len(positions), dtype=pkg.Context.MIXED_ROW_DTYPE)
        paths = np.zeros((len(positions), mp), dtype=pkg.Context.MIXED_DTYPE)
        for i, S in enumerate(positions):
            r, ps = self.row(S, L, NO_OBJECT if src_obj is None else src_obj[i], lis_obj, **params)
            for k in rows.dtype.names:
                rows[i][k] = r[k]
            for j, y in enumerate(ps[:mp]):
                for k in paths.dtype.names:
                    paths[i, j][k] = y[k]
        return rows, paths


# ---- the scene ------------------------------------------------------------------------------------------------------
SIZE = 1000.0
SRC, LIS = [250.0, 200.0, 150.0], [750.0, 200.0, 150.0]
LIS2 = [620.0, 350.0, 380.0]    # off the symmetry of SRC and LIS: the floor and the ceiling bounce bend at the rim's inside
WIDTH = 600.0
CENTRE = (500.0, 500.0)
X0, X1, Y0, Y1, FLOOR, CEILING, PARTITION = range(7)   # the reflectors: box()'s wall order, then the partition
# fp32 against float64: the chain of test_diffraction_paths.py (about forty roundings for its 2e-5) behind the image — A - v0, the dot,
# 2 hA / nn, k n and the subtraction, about ten more
LENGTH_RTOL = 2e-5 * 50 / 40
POINT_ATOL = LENGTH_RTOL * SIZE * 10   # apex and reflection point: the figure on the room's size, times ten, as the existing path tests
# The rule's R is where the leg from EA meets the reflector, and EA stands `offset` off the apex along o and along n: R lies within
# sqrt(2) offset of the model's point, and the direction towards it (end 0) turns by at most that over the leg's length
OFF_APEX = np.sqrt(2.0) * DEFAULTS["offset"]


def turned(points, degrees):
    """the points turned about the vertical through CENTRE, in float64"""
    p = np.array(points, np.float64)
    if degrees:
        t = np.deg2rad(degrees)
        x, y = p[..., 0] - CENTRE[0], p[..., 1] - CENTRE[1]
        p[..., 0], p[..., 1] = CENTRE[0] + np.cos(t) * x - np.sin(t) * y, CENTRE[1] + np.sin(t) * x + np.cos(t) * y
    return p


def scene_world(n=1, degrees=0.0, width=WIDTH, extra=(), actor=2, material=OPAQUE, tables=(ALPHA, TAU, 4, SCAT)):
    """the room's 12 n^2 triangles, then the partition's 2 n^2, then the extras (triangles, material, actor)"""
    parts = [(box([0.0, 0.0, 0.0], [SIZE] * 3, n), WALLS, 1), (quad_grid((500.0, 0.0, 0.0), (0.0, width, 0.0), (0.0, 0.0, SIZE), n), material, actor)]
    parts = [(turned(t, degrees), m, a) for t, m, a in parts + list(extra)]
    return World(parts, tables[0], tables[1], tables[2], tables[3])


def reflector_of(triangle, n):
    return int(triangle) // (2 * n * n)


class Model:
    """float64, independent of the rule's arithmetic: the scene as seven parallelograms and one rim line"""

    def __init__(self, degrees=0.0, width=WIDTH):
        s = SIZE
        quads = [((0, 0, 0), (0, s, 0), (0, 0, s)), ((s, 0, 0), (0, s, 0), (0, 0, s)), ((0, 0, 0), (s, 0, 0), (0, 0, s)), ((0, s, 0), (s, 0, 0), (0, 0, s)),
                 ((0, 0, 0), (s, 0, 0), (0, s, 0)), ((0, 0, s), (s, 0, 0), (0, s, 0)), ((500, 0, 0), (0, width, 0), (0, 0, s))]
        self.quads = []
        for o, du, dv in quads:
            o, du, dv = (np.asarray(x, np.float64) for x in (o, du, dv))
            c = turned([o, o + du, o + dv], degrees)
            self.quads.append((c[0], c[1] - c[0], c[2] - c[0]))
        po, pdu, pdv = self.quads[PARTITION]
        self.a, self.w = po + pdu, pdv                     # the free rim
        self.out = pdu / np.linalg.norm(pdu)               # in the partition's plane, away from its inside
        self.pn = np.cross(pdu, pdv) / np.linalg.norm(np.cross(pdu, pdv))
        self.degrees = degrees
        self.free = width < SIZE                           # a rim that lies in the wall y = 1000 is no rim

    def place(self, P):
        return turned(P, self.degrees)

    @staticmethod
    def inside(quad, P, slack=0.0):
        o, du, dv = quad
        u, v = np.dot(P - o, du) / np.dot(du, du), np.dot(P - o, dv) / np.dot(dv, dv)
        return slack < u < 1 - slack and slack < v < 1 - slack

    def cut(self, P, Q, blockers=()):
        """the open segment P -> Q passes through the partition's or a blocker's inside (a point in its plane is not cut by it)"""
        for quad in [self.quads[PARTITION]] + list(blockers):
            o, du, dv = quad
            nrm = np.cross(du, dv)
            hP, hQ = np.dot(P - o, nrm), np.dot(Q - o, nrm)
            tiny = 1e-7 * np.linalg.norm(nrm)
            if abs(hP) <= tiny or abs(hQ) <= tiny or hP * hQ > 0:
                continue
            if self.inside(quad, P + hP / (hP - hQ) * (Q - P)):
                return True
        return False

    def paths(self, S, L, max_length=2000.0, max_detour=1000.0, blockers=()):
        S, L = np.asarray(S, np.float64), np.asarray(L, np.float64)
        out = []
        for end in (0, 1) if self.free else ():
            A, Z = (S, L) if end else (L, S)
            for k, (o, du, dv) in enumerate(self.quads):
                n = np.cross(du, dv) / np.linalg.norm(np.cross(du, dv))
                hA = np.dot(A - o, n)
                if abs(hA) < 1e-9:
                    continue
                A1 = A - 2.0 * hA * n                                         # mirror the end in the plane
                wl = np.linalg.norm(self.w)
                wh = self.w / wl
                tA, tZ = np.dot(A1 - self.a, wh), np.dot(Z - self.a, wh)      # unfold about the rim's line
                dA, dZ = np.linalg.norm(np.cross(A1 - self.a, wh)), np.linalg.norm(np.cross(Z - self.a, wh))
                along = tA + (tZ - tA) * dA / (dA + dZ)
                if not 0.0 < along < wl:
                    continue
                E = self.a + along * wh
                length = float(np.hypot(dA + dZ, tZ - tA))
                unfolded = float(np.linalg.norm(A1 - Z))
                if length > max_length or length - unfolded > max_detour:
                    continue
                h1, hZ = np.dot(A1 - self.a, self.pn), np.dot(Z - self.a, self.pn)
                if h1 * hZ >= 0:
                    continue                                                  # both on one side: nothing to bend round
                X = A1 + h1 / (h1 - hZ) * (Z - A1)
                if np.dot(X - E, self.out) > 0:
                    continue                                                  # the unfolded segment passes the rim lit
                D = A1 - E                                                    # intersect the plane
                if np.dot(D, n) == 0:
                    continue
                s = np.dot(o - E, n) / np.dot(D, n)
                if not 1e-12 < s < 1.0:
                    continue
                R = E + s * D
                if not self.inside((o, du, dv), R):
                    continue
                if self.cut(Z, E, blockers) or self.cut(E, R, blockers) or self.cut(R, A, blockers):
                    continue
                out.append(dict(end=end, reflector=k, length=length, E=E, R=R, A=A, Z=Z, A1=A1, unfolded=unfolded, along=along / wl))
        return out


def check_path(p, ref, S, L, gm):
    """a restatement's path against the model's, the tolerances of the existing path tests scaled by the path's length"""
    length = ref["length"]
    assert abs(float(p["length"]) - length) <= LENGTH_RTOL * length, (p["length"], length)
    assert np.allclose(p["apex"], ref["E"], rtol=0, atol=POINT_ATOL) and np.allclose(p["point"], ref["R"], rtol=0, atol=POINT_ATOL + OFF_APEX)
    straight = float(np.linalg.norm(np.asarray(S, np.float64) - np.asarray(L, np.float64)))
    assert p["detour"] > 0 and abs(float(p["detour"]) - (length - straight)) <= 2 * LENGTH_RTOL * length
    bend = length - ref["unfolded"]
    assert p["bend_detour"] > 0 and abs(float(p["bend_detour"]) - bend) <= 2 * LENGTH_RTOL * length
    first = ref["E"] if ref["end"] else ref["R"]
    d = (first - np.asarray(L, np.float64)) / np.linalg.norm(first - np.asarray(L, np.float64))
    assert np.allclose(p["direction"], d, rtol=0, atol=1e-4 + (0.0 if ref["end"] else OFF_APEX / np.linalg.norm(first - np.asarray(L, np.float64))))
    a, b = ref["E"] - (ref["A1"] if ref["end"] else ref["Z"]), (ref["Z"] if ref["end"] else ref["A1"]) - ref["E"]   # S' -> E, E -> L'
    assert abs(float(p["cos_bend"]) - float(np.dot(a, b) / np.linalg.norm(a) / np.linalg.norm(b))) <= 1e-5
    g = p["gain"]
    k = [40.0 * f / (343.0 * 1000.0) for f in (125.0, 250.0, 500.0, 1000.0)]
    assert np.all(g[:4] > 0) and np.all(g[4:] == 0)
    assert np.allclose(g[:4], [float(gm[b]) / np.sqrt(3.0 + k[b] * bend) for b in range(4)], rtol=1e-4)
    assert int(p["end"]) == ref["end"]


def match(paths, refs, n, S, L, y):
    """every path of the model is matched by one of the restatement's, and there is no other"""
    assert len(paths) == len(refs), ([(int(p["end"]), reflector_of(p["triangle"][0], n), float(p["length"])) for p in paths],
                                     [(r["end"], r["reflector"], r["length"]) for r in refs])
    left = list(paths)
    for ref in refs:
        mine = [p for p in left if int(p["end"]) == ref["end"] and reflector_of(p["triangle"][0], n) == ref["reflector"]]
        assert len(mine) == 1, (ref["end"], ref["reflector"], len(mine))
        check_path(mine[0], ref, S, L, y.reflectance(int(mine[0]["triangle"][0])))
        assert reflector_of(mine[0]["triangle"][1], n) == PARTITION, "the edge is the partition's"
        left = [p for p in left if p is not mine[0]]
    assert not left


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.MixedParams) == 52 and C.sizeof(cap.MixedPath) == 112 and C.sizeof(cap.MixedRow) == 24
    assert pkg.Context.MIXED_DTYPE.itemsize == 112 and pkg.Context.MIXED_ROW_DTYPE.itemsize == 24
    P = cap.MixedPath
    names = ("length", "delay", "detour", "bend_detour", "cos_bend", "apex", "point", "direction", "end", "triangle", "edge", "material", "gain")
    offsets = [0, 4, 8, 12, 16, 20, 32, 44, 56, 60, 68, 72, 80]
    assert [getattr(P, k).offset for k in names] == offsets
    assert pkg.Context.MIXED_DTYPE.names == names and [pkg.Context.MIXED_DTYPE.fields[k][1] for k in names] == offsets
    assert pkg.Context.MIXED_ROW_DTYPE.names == ("near", "candidates", "confirmed", "found", "returned", "flags")
    assert [k for k, _ in cap.MixedRow._fields_] == ["near", "candidates", "confirmed", "found", "returned", "flags"]
    assert [k for k, _ in cap.MixedParams._fields_] == ["struct_size"] + list(DEFAULTS)
    p = cap.default_mixed_params()
    assert p.struct_size == 52
    for k, v in DEFAULTS.items():
        assert getattr(p, k) == (F(v) if isinstance(v, float) else v), k
    assert (cap.MAX_MIXED_PATHS, cap.MAX_MIXED_NEAR, cap.MAX_MIXED_CANDIDATES, cap.MAX_MIXED_BATCH, cap.MIXED_OVERFLOW, cap.MIXED_NEAR_OVERFLOW,
            cap.MIXED_VOICE_TAG) == (16, 32768, 2048, 256, 1, 2, TAG)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frequensee.h")).read()
    for name, value in (("FS_MAX_MIXED_PATHS", "16"), ("FS_MAX_MIXED_NEAR", "32768"), ("FS_MAX_MIXED_CANDIDATES", "2048"), ("FS_MAX_MIXED_BATCH", "256"),
                        ("FS_MIXED_OVERFLOW", "1u"), ("FS_MIXED_NEAR_OVERFLOW", "2u")):
        assert f"#define {name}" in header and header.split(f"#define {name}")[1].split()[0] == value
    assert cap.load().fs_abi_version() == 5, "the change only adds"
    # the keys: above every first-order diffraction key of a scene of fewer than 2^28 triangles, and so above every other kind's
    assert TAG > cap.DIFFRACTION_VOICE_TAG | (4 * (2 ** 28 - 1) + 2) and cap.DIFFRACTION_VOICE_TAG | (4 * 2 ** 28) == TAG
    assert cap.DIFFRACTION_VOICE_TAG > cap.REFLECTION2_VOICE_TAG > cap.DIFFRACTION2_VOICE_TAG
    for tri, edge, end in (([0, 0], 0, 0), ([2 ** 28 - 1, 2 ** 28 - 1], 2, 1), ([12345, 678], 1, 1)):
        key = voice_key(dict(triangle=tri, edge=edge, end=end))
        assert TAG <= key < 2 ** 32 and key == pkg.FrequenSeeAudioReflectionPlugin.MixedKey(tri, edge, end)
    assert voice_key(dict(triangle=[1, 0], edge=0, end=0)) == TAG | (2654435761 >> 2)
    # the end and the edge survive the shift: the two ends of one (reflector, edge record) have different keys
    assert len({voice_key(dict(triangle=[4, 13], edge=j, end=end)) for j in range(3) for end in (0, 1)}) == 6


def test_exported_in_one_tier(pkg):
    contract.exported_in_one_tier(pkg, ("fs_mixed_params_default", "fs_update_mixed_paths"))


def test_null_context_and_no_device(pkg):
    contract.null_context_and_no_device(pkg, QUERY)


def test_model_figures():
    """the closed forms the float64 model is held to"""
    by = {(r["end"], r["reflector"]): r for r in Model().paths(SRC, LIS)}
    assert sorted(by) == [(0, X1), (0, Y0), (1, X0), (1, Y0)], sorted(by)
    behind = by[1, X0]
    assert abs(behind["length"] - (np.sqrt(250.0 ** 2 + 400.0 ** 2) + 850.0)) < 1e-9 and abs(behind["length"] - 1321.699) < 5e-4
    assert np.allclose(behind["R"], (0.0, 1000.0 / 3.0, 150.0), atol=1e-9) and np.allclose(behind["E"], (500.0, 600.0, 150.0), atol=1e-9)
    mirror = by[0, X1]
    assert abs(mirror["length"] - behind["length"]) < 1e-9 and np.allclose(mirror["R"], (1000.0, 1000.0 / 3.0, 150.0), atol=1e-9)
    for end, x in ((1, 312.5), (0, 687.5)):
        assert abs(by[end, Y0]["length"] - (np.hypot(250.0, 800.0) + np.hypot(250.0, 400.0))) < 1e-9
        assert np.allclose(by[end, Y0]["R"], (x, 0.0, 150.0), atol=1e-9)
    # the wall y = 1000: the unfolded segment passes the rim lit; the partition's own faces: the apex lies in the reflector's plane.
    # The floor and the ceiling: the unfolded segment meets the rim's line at its very foot and head (see the module's docstring)
    S1 = np.array([250.0, 200.0, -150.0])
    dA, dZ = np.hypot(250.0, 400.0), np.hypot(250.0, 400.0)
    assert -150.0 + 300.0 * dA / (dA + dZ) == 0.0 and S1[2] == -150.0
    # off the symmetry every wall but y = 1000 carries a path for at least one end, the floor and the ceiling among them
    by2 = {(r["end"], r["reflector"]) for r in Model().paths(SRC, LIS2)}
    assert {k for _, k in by2} == {X0, X1, Y0, FLOOR, CEILING} and len(by2) >= 6, sorted(by2)
    for n in (1, 2, 4):   # (on the input) no apex near the end of a sub-edge of the rim
        for r in Model().paths(SRC, LIS) + Model().paths(SRC, LIS2) + Model().paths(LIS2, SRC):
            t = r["along"] * n
            assert min(t - np.floor(t), np.ceil(t) - t) > 0.02, (n, r["end"], r["reflector"], r["along"])


CASES = {"the scene": (SRC, LIS, 0.0), "ends swapped": (LIS, SRC, 0.0), "turned 17 degrees": (SRC, LIS, 17.0),
         "off the symmetry": (SRC, LIS2, 0.0), "off the symmetry, ends swapped": (LIS2, SRC, 0.0), "off the symmetry, turned": (SRC, LIS2, 17.0)}


@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_against_model(pkg, oracle_mod, case, n):
    S, L, degrees = CASES[case]
    model = Model(degrees)
    S, L = model.place(S), model.place(L)
    refs = model.paths(S, L)
    assert len(refs) >= 4
    w = scene_world(n, degrees)
    assert len(w.tri) == 14 * n * n
    y = Mixed(oracle_mod, w)
    r, paths = y.row(S, L, max_paths=16, **REACH)
    assert r["flags"] == 0 and r["near"] <= 4 * len(w.tri) and r["candidates"] >= r["confirmed"] >= r["found"] == len(paths), r
    match(paths, refs, n, S, L, y)
    assert [bits(p["length"]) for p in paths] == sorted(bits(p["length"]) for p in paths)
    assert len({voice_key(p) for p in paths}) == len(paths)
    if n > 1:
        assert y.mx["blocked"][1] > 0, "no interior edge was rejected by the short leg"
    if case == "the scene":
        lengths = {(int(p["end"]), reflector_of(p["triangle"][0], n)): float(p["length"]) for p in paths}
        assert abs(lengths[1, X0] - 1321.699) < 0.05 and abs(lengths[0, X1] - 1321.699) < 0.05
        # the default max_length looks 500 cm far: nothing of this room
        assert y.row(S, L)[0]["found"] == 0


def test_restatement_partition_to_full_width(pkg, oracle_mod):
    y = Mixed(oracle_mod, scene_world(2, width=SIZE))
    r, paths = y.row(SRC, LIS, **REACH)
    assert r["found"] == 0 and not paths and r["near"] > 0
    assert not Model(width=SIZE).paths(SRC, LIS)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
check = contract.checker("mixed")


def identities(paths):
    """what a path is from scene to scene: its end, its reflector and its edge record"""
    return {(int(p["end"]), int(p["triangle"][0]), int(p["triangle"][1]), int(p["edge"])) for p in paths}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4], ids=["14_triangles", "224_triangles"])
def test_scene(pkg, oracle_mod, n):
    """n = 1: one workgroup of held entries, one partly full tile; n = 4: four of each"""
    w = scene_world(n)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, paths = check(pkg, ctx, Mixed(oracle_mod, w), h, [SRC], LIS, f"scene n={n}", **REACH)
    assert rows[0]["near"] > 3 * len(w.tri) and tuple(rows[0])[3:] == (4, 4, 0) and rows[0]["confirmed"] >= 4
    assert np.all(paths[0][4:].view(np.uint8) == 0)
    assert sorted((int(p["end"]), reflector_of(p["triangle"][0], n)) for p in paths[0][:4]) == [(0, X1), (0, Y0), (1, X0), (1, Y0)]
    check(pkg, ctx, Mixed(oracle_mod, w), h, [SRC], LIS, f"scene n={n}, defaults")
    assert ctx.mixed_paths(h)[0][0]["found"] == 0, "the default max_length"
    h2 = place(ctx, [SRC, LIS2])
    ctx.set_listener(LIS2)
    rows, _ = check(pkg, ctx, Mixed(oracle_mod, w), h2, [SRC, LIS2], LIS2, f"scene n={n}, second listener", max_paths=16, **REACH)
    assert rows[0]["found"] >= 6 and rows[1]["found"] == 0
    ctx.close()


# ---- near lists that end at the edges of the pair kernel's tiles ---------------------------------------------------------
# The pair kernel streams a row's near list through LDS in tiles of 256 entries, shared among at most 16 workgroups per tile of held
# entries: a list of 255, 256 and 257 entries ends one entry either side of a tile's edge, one of 4100 has 17 tiles.
TILE_EDGE_NEAR = (255, 256, 257, 4100)
_tile_edges = {}


def sparse_field(count):
    """count triangles of about 1 cm, 11 cm apart under the ceiling, each turned a little further about z, as
    test_diffraction2_paths.py builds its field, with sides of three lengths so that a triangle's face and its three edge records
    have four different near bounds: every one adds four entries between 1500 and 1800 cm"""
    k = np.arange(count)
    v0 = np.stack([240.0 + 11.0 * (k % 48), 20.0 + 11.0 * (k // 48), np.full(count, 900.0)], axis=1)
    a = 0.3 + 0.9 * k / max(count, 1)
    e1 = np.stack([np.cos(a), np.sin(a), np.zeros(count)], axis=1)
    e2 = 1.3 * np.stack([-np.sin(a), np.cos(a), np.zeros(count)], axis=1)
    return np.stack([v0, v0 + e1, v0 + e2], axis=1).astype(np.float32)


def tile_edge_case(pkg, oracle_mod, near):
    """(world, max_length, the call's two arrays by the restatement): the scene with a sparse field of more faces and edge records
    than asked for, and the max_length that lies between the near bounds of entry number `near` and the next — computed once"""
    if near not in _tile_edges:
        w = scene_world(extra=[(sparse_field(near // 4 + 24), OPAQUE, 3)])
        y = Mixed(oracle_mod, w)
        S32, L32 = np.asarray(SRC, np.float32), np.asarray(LIS, np.float32)
        with np.errstate(all="ignore"):
            a, b = S32[None, :] - y.v0, L32[None, :] - y.v0
            reach = np.maximum(np.sqrt(dot(y.e1, y.e1)), np.sqrt(dot(y.e2, y.e2)))
            face = (np.sqrt(dot(a, a)) + np.sqrt(dot(b, b))) - (reach + reach)
            rS, rL, er = S32[None, :] - y.ra, L32[None, :] - y.ra, np.sqrt(y.rww)
            edge = (np.sqrt(dot(rS, rS)) + np.sqrt(dot(rL, rL))) - (er + er)
        need = np.sort(np.concatenate([face, edge]))
        assert need.dtype == np.float32 and len(need) > near and need[near] - need[near - 1] > 1e-3, "no max_length cuts the list there"
        length = float(need[near - 1]) + 0.5 * float(need[near] - need[near - 1])
        assert length > 1400.0, "the scene's own paths would be cut"
        _tile_edges[near] = w, length, y.expect(pkg, [SRC], LIS, max_length=length)
    return _tile_edges[near]


@pytest.mark.parametrize("near", TILE_EDGE_NEAR)
def test_tile_edge_preconditions(pkg, oracle_mod, near):
    """the restatement alone: the near list has the length asked for and the scene's four paths are found"""
    rows, paths = tile_edge_case(pkg, oracle_mod, near)[2]
    assert rows[0]["near"] == near and rows[0]["candidates"] >= 4 and rows[0]["returned"] >= 4 and rows[0]["flags"] == 0
    assert np.all(paths[0]["length"][:rows[0]["returned"]] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("near", TILE_EDGE_NEAR)
def test_near_list_at_tile_edges(pkg, oracle_mod, near):
    w, length, want = tile_edge_case(pkg, oracle_mod, near)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    got = ctx.mixed_paths(place(ctx, [SRC]), max_length=length)
    assert_equal(got, want, f"near list of {near}")
    assert got[0][0]["near"] == near and got[0][0]["returned"] >= 4
    ctx.close()


# The path behind the source: S -> R = (0, 333.3, 150) on the wall x = 0 -> E = (500, 600, 150) -> L.  A small quad across each of its
# legs, and the (end, reflector) of the paths that run through that leg (see the module's docstring).
BLOCKERS = {
    "leg 1": (quad_grid((600.0, 400.0, 100.0), (50.0, 0.0, 0.0), (0.0, 0.0, 100.0), 1), {(1, X0), (1, Y0)}),            # between the rim and L
    "leg 2": (quad_grid((500.05, 600.05, 100.0), (0.0, 30.0, 0.0), (0.0, 0.0, 100.0), 1),                                # a lip beside the rim,
              {(1, X0), (1, Y0), (0, X1), (0, Y0)}),                                                                     # off the partition
    "leg 3": (quad_grid((250.0, 440.0, 100.0), (0.0, 50.0, 0.0), (0.0, 0.0, 100.0), 1), {(1, X0)}),                     # between the rim and R
    "leg 4": (quad_grid((125.0, 240.0, 100.0), (0.0, 50.0, 0.0), (0.0, 0.0, 100.0), 1), {(1, X0)}),                     # between R and S
}


def behind_the_source(c):
    return c["end"] == 1 and reflector_of(c["m"], 1) == X0 and reflector_of(c["r"] // 3, 1) == PARTITION and \
        abs(float(c["E"][1]) - WIDTH) < 1e-2 and abs(float(c["E"][2]) - 150.0) < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("leg", sorted(BLOCKERS))
def test_each_leg_blocked(pkg, oracle_mod, leg):
    quad, gone = BLOCKERS[leg]
    clear = Mixed(oracle_mod, scene_world(1))
    full = clear.row(SRC, LIS, **REACH)[1]
    assert len(full) == 4
    w = scene_world(1, extra=[(quad, OPAQUE, 3)])
    y = Mixed(oracle_mod, w)
    # (on the restatement) the path behind the source is still a candidate, and of its four legs the one meant fails and no other
    # (leg 4 exists only behind leg 3)
    S32, L32 = np.asarray(SRC, np.float32), np.asarray(LIS, np.float32)
    faces, edges = y.near_sets(S32, L32, set(), REACH["max_length"])
    target = [c for c in y.triples(S32, L32, faces, edges, dict(DEFAULTS, **REACH)) if behind_the_source(c)]
    assert len(target) == 1
    verdict = y.legs(list(S32), list(L32), set(), target[0], dict(DEFAULTS, **REACH), stop_at_first=False)[0]
    assert [k for k in (1, 2, 3, 4) if not verdict.get(k, True)] == [int(leg[-1])], verdict
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, y, place(ctx, [SRC]), [SRC], LIS, leg, max_paths=16, **REACH)
    got = identities(paths[0][:rows[0]["returned"]])
    for p in full:
        one = (int(p["end"]), int(p["triangle"][0]), int(p["triangle"][1]), int(p["edge"]))
        assert (one in got) == ((one[0], reflector_of(one[1], 1)) not in gone), (leg, one)
    ctx.close()


@pytest.mark.gpu
def test_full_width_and_own_actors(pkg, oracle_mod):
    w = scene_world(2, width=SIZE)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Mixed(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, "to full width", **REACH)
    assert rows[0]["found"] == 0 and rows[0]["near"] > 0 and np.all(paths.view(np.uint8) == 0)
    ctx.close()
    # the blocker between R and S as the source's own actor, the one between the rim and L as the listener's: the legs pass them,
    # their triangles are never near; under foreign ids they block
    extra = [(BLOCKERS["leg 4"][0], OPAQUE, 7), (BLOCKERS["leg 1"][0], OPAQUE, 8)]
    w = scene_world(1, extra=extra)
    y = Mixed(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "foreign ids", max_paths=16, **REACH)
    seen = {(int(p["end"]), reflector_of(p["triangle"][0], 1)) for p in paths[0][:rows[0]["returned"]]}
    assert (1, X0) not in seen and (1, Y0) not in seen and {(0, X1), (0, Y0)} <= seen
    near = int(rows[0]["near"])
    ctx.set_source_object(h[0], 7)
    ctx.set_listener_object(8)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "own actors at both ends", src_obj=[7], lis_obj=8, max_paths=16, **REACH)
    assert rows[0]["near"] == near - 16 and rows[0]["found"] == 4 and y.stats["passed_own"] > 0
    assert {(int(p["end"]), reflector_of(p["triangle"][0], 1)) for p in paths[0][:4]} == {(0, X1), (0, Y0), (1, X0), (1, Y0)}
    ctx.close()
    # the partition as the source's own actor: no edge of it is near, and the room has no other free edge
    w = scene_world(1)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    ctx.set_source_object(h[0], 2)
    rows, _ = check(pkg, ctx, Mixed(oracle_mod, w), h, [SRC], LIS, "the partition as an own actor", src_obj=[2], **REACH)
    assert rows[0]["near"] == 48 and rows[0]["found"] == 0
    ctx.close()


@pytest.mark.gpu
def test_caps(pkg, oracle_mod):
    w = scene_world(2)
    y = Mixed(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    full = ctx.mixed_paths(h, **REACH)
    near, cands, confirmed = (int(full[0][0][k]) for k in ("near", "candidates", "confirmed"))
    assert near > 100 and cands >= confirmed >= 4 and tuple(full[0][0])[3:] == (4, 4, 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "near exactly at the cap", max_near=near, **REACH)
    assert rows.tobytes() == full[0].tobytes() and paths.tobytes() == full[1].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "near overflow", max_near=near - 1, **REACH)
    assert tuple(rows[0]) == (near, 0, 0, 0, 0, NEAR_OVERFLOW) and np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "candidates exactly at the cap", max_candidates=cands, max_paths=16, **REACH)
    assert tuple(rows[0]) == tuple(full[0][0]) and paths.shape == (1, 16) and np.all(paths[0][4:].view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "candidate overflow", max_candidates=cands - 1, **REACH)
    assert tuple(rows[0]) == (near, cands, 0, 0, 0, OVERFLOW) and np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "paths exactly at the cap", max_paths=4, **REACH)
    assert tuple(rows[0]) == tuple(full[0][0]) and paths.tobytes() == full[1][0][:4].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "the three shortest", max_paths=3, **REACH)
    assert tuple(rows[0])[3:] == (4, 3, 0) and paths.shape == (1, 3) and paths[0].tobytes() == full[1][0][:3].tobytes()
    # max_detour and max_length just above and just below the shortest path's: it is in, then out
    first = full[1][0][0]
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "length cap above", max_length=float(first["length"]) * (1.0 + 1e-5))
    assert rows[0]["found"] >= 1 and paths[0][0].tobytes() == first.tobytes() and rows[0]["near"] <= near
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "length cap below", max_length=float(first["length"]) * (1.0 - 1e-5))
    assert rows[0]["found"] == 0
    bend = float(max(full[1][0][:4]["bend_detour"]))
    rows, _ = check(pkg, ctx, y, h, [SRC], LIS, "detour cap above", max_detour=bend * (1.0 + 1e-5), **REACH)
    assert rows[0]["found"] == 4
    rows, _ = check(pkg, ctx, y, h, [SRC], LIS, "detour cap below", max_detour=bend * (1.0 - 1e-5), **REACH)
    assert rows[0]["found"] == 2
    rows, _ = check(pkg, ctx, y, h, [SRC], LIS, "merge 0", merge=0.0, **REACH)
    assert rows[0]["found"] == rows[0]["confirmed"] >= 4
    ctx.close()


ALPHA8 = [[0.5, 0.4, 0.3, 0.2, 0.3, 0.4, 0.5, 0.6], [0.6, 0.5, 0.7, 0.4, 0.2, 0.3, 0.1, 0.5], [0.9] * 8]
TAU8 = [[0.05, 0.1, 0.02, 0.0, 0.1, 0.0, 0.05, 0.1], [0.3, 0.25, 0.5, 0.4, 0.1, 0.2, 0.05, 0.3], [0.0] * 8]
SCAT8 = [[0.2, 0.3, 0.4, 0.5, 0.6, 0.5, 0.4, 0.3], [0.1, 0.6, 0.3, 0.9, 0.5, 0.2, 0.7, 0.4], [0.5] * 8]


@pytest.mark.gpu
def test_materials_degenerate_triangles_and_bands(pkg, oracle_mod):
    room = box([0.0, 0.0, 0.0], [SIZE] * 3)
    part = quad_grid((500.0, 0.0, 0.0), (0.0, WIDTH, 0.0), (0.0, 0.0, SIZE), 1)
    degenerate = np.array([[[450.0, 100.0, 250.0], [450.0, 100.0, 250.0], [450.0, 300.0, 260.0]],      # two corners equal
                           [[550.0, 0.0, 210.0], [550.0, 200.0, 230.0], [550.0, 400.0, 250.0]],        # three on a line
                           [[500.0, 300.0, 220.0], [500.0, 300.0, 220.0], [500.0, 300.0, 220.0]]], np.float32)   # a point
    # the wall x = 0: no material; x = 1000: an id beyond the table; the rest: material 0; three bands
    w = World([(room[0:2], NO_MATERIAL, 1), (room[2:4], 9, 1), (room[4:12], 0, 1), (part, 1, 2), (degenerate, 0, 2)],
              [a[:3] for a in ALPHA], [t[:3] for t in TAU], 3, [x[:3] for x in SCAT])
    y = Mixed(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "materials", **REACH)
    assert tuple(rows[0])[3:] == (4, 4, 0), "a degenerate triangle was in the way"
    by = {(int(p["end"]), reflector_of(p["triangle"][0], 1)): p for p in paths[0][:4]}
    assert tuple(int(m) for m in by[1, X0]["material"]) == (NO_MATERIAL, 1) and tuple(int(m) for m in by[0, X1]["material"]) == (9, 1)
    assert by[1, X0]["gain"].tobytes() == by[0, X1]["gain"].tobytes(), "neither reflector applies a factor"
    assert int(by[1, Y0]["material"][0]) == 0 and np.all(by[1, Y0]["gain"][:3] < by[1, X0]["gain"][:3] * 1.001) and np.all(by[1, Y0]["gain"][:3] > 0)
    for p in paths[0][:4]:
        assert np.all(p["gain"][3:] == 0)
    for k in ("length", "delay", "detour", "bend_detour", "cos_bend", "apex", "point", "direction", "gain"):
        assert np.all(np.isfinite(paths[k]))
    edges = [300.0, 1200.0]
    ctx.set_band_edges(edges)
    check(pkg, ctx, Mixed(oracle_mod, w, edges=edges), h, [SRC], LIS, "edges given", **REACH)
    ctx.set_band_edges(None)
    check(pkg, ctx, y, h, [SRC], LIS, "default edges again", **REACH)
    ctx.close()
    for tables in (([[0.5]], [[0.0]], 1, [[0.5]]), (ALPHA8, TAU8, 8, SCAT8)):
        w = scene_world(1, tables=tables)
        ctx = w.context(pkg)
        ctx.set_listener(LIS)
        rows, paths = check(pkg, ctx, Mixed(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, f"{tables[2]} bands", **REACH)
        B = tables[2]
        assert rows[0]["found"] == 4 and np.all(paths[0]["gain"][:4, :B] > 0) and np.all(paths[0]["gain"][:, B:] == 0)
        ctx.close()


_builders = {}


def builders_case(pkg, oracle_mod):
    """the scene at n = 4, nine sources — SRC, LIS2 and seven seeded ones on SRC's side — against LIS: the restatement's arrays, once"""
    if not _builders:
        w = scene_world(4)
        pos = np.random.default_rng(0x313D).uniform([60.0, 60.0, 60.0], [440.0, 560.0, 900.0], (9, 3)).astype(np.float32)
        pos[0], pos[1] = SRC, LIS2
        _builders.update(w=w, pos=pos, want=Mixed(oracle_mod, w).expect(pkg, pos, LIS, max_length=1500.0))
    return _builders


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["sah", "device_morton"])
def test_both_tree_builders(pkg, oracle_mod, fast):
    bc = builders_case(pkg, oracle_mod)
    wrows = bc["want"][0]
    assert not np.any(wrows["flags"]) and np.count_nonzero(wrows["returned"]) >= 5 and np.any(wrows["confirmed"] < wrows["candidates"]), wrows
    ctx = bc["w"].context(pkg, fast=fast)
    ctx.set_listener(LIS)
    h = place(ctx, bc["pos"])
    rows, paths = got = ctx.mixed_paths(h, max_length=1500.0)
    assert_equal(got, bc["want"], f"builders fast={fast}")
    contract.batch_agrees(ctx.mixed_paths, h, got, singles=not fast, max_length=1500.0)
    ctx.close()


@pytest.mark.gpu
def test_mover(pkg, oracle_mod):
    """a door in the partition's plane shuts the gap beside the rim: no path; the door slid out of the room: the scene's four; the
    door back: none"""
    door = quad_grid((500.0, WIDTH, 0.0), (0.0, SIZE - WIDTH, 0.0), (0.0, 0.0, SIZE), 1)
    w = scene_world(1, extra=[(door, OPAQUE, 5)])
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, _ = check(pkg, ctx, Mixed(oracle_mod, w), h, [SRC], LIS, "door shut", **REACH)
    assert rows[0]["found"] == 0
    aside = np.array([[1, 0, 0, 0], [0, 1, 0, 2000], [0, 0, 1, 0]], np.float32)
    ctx.set_object_transforms([5], aside[None])
    rows, _ = check(pkg, ctx, Mixed(oracle_mod, w, contract.transformed(w, 5, aside)), h, [SRC], LIS, "door aside, no explicit refit", **REACH)   # the call refits first
    assert rows[0]["found"] == 4
    ctx.set_object_transforms([5], np.eye(3, 4, dtype=np.float32)[None])
    rows, _ = check(pkg, ctx, Mixed(oracle_mod, w), h, [SRC], LIS, "door back", **REACH)
    assert rows[0]["found"] == 0
    ctx.close()


def _defaults_found(t, oracle_mod, want):
    y = Mixed(oracle_mod, t.w)
    assert_equal(want, y.expect(t.pkg, [SRC, SRC], LIS), "defaults, one handle twice")
    assert_equal(t.ctx.mixed_paths([t.src, t.src], **REACH), y.expect(t.pkg, [SRC, SRC], LIS, **REACH), "one handle twice")


def _legal_found(rows):
    assert tuple(rows[0])[2:] == (0, 0, 0, OVERFLOW) and rows[0]["candidates"] > 1


def _untouched_found(got):
    assert got[0][0]["found"] == 4


def _steady_found(ctx, h, first, fewer):
    assert np.all(first[0]["found"] == 4)


inf, nan = float("inf"), float("nan")
QUERY = contract.Query(
    kind="mixed", dtypes=("MIXED_ROW_DTYPE", "MIXED_DTYPE"), world=lambda: scene_world(1), src=SRC, lis=LIS, wrong_struct_size=44, reach=REACH,
    refused_without_device=(dict(max_detour=0.0), dict(max_length=0.0), dict(max_near=0), dict(max_paths=17)),
    refused=(dict(max_paths=0), dict(max_paths=17), dict(max_near=0), dict(max_near=32769), dict(max_candidates=0), dict(max_candidates=2049),
             dict(max_length=0.0), dict(max_length=-1.0), dict(max_length=nan), dict(max_length=inf), dict(max_detour=0.0), dict(max_detour=-1.0),
             dict(max_detour=nan), dict(max_detour=inf), dict(margin=-1e-3), dict(margin=nan), dict(margin=inf), dict(offset=-0.1), dict(offset=nan),
             dict(offset=inf), dict(merge=-1.0), dict(merge=nan), dict(merge=inf), dict(step=-0.1), dict(step=nan), dict(step=inf),
             dict(pullback=-1.0), dict(pullback=nan), dict(pullback=inf), dict(dist_divisor=0.0), dict(dist_divisor=-1.0), dict(dist_divisor=nan),
             dict(dist_divisor=inf), dict(sound_speed=0.0), dict(sound_speed=-1.0), dict(sound_speed=nan), dict(sound_speed=inf)),
    defaults_found=_defaults_found,
    legal=(dict(max_paths=16, max_near=32768, max_candidates=2048, margin=0.0, offset=0.0, merge=0.0, step=0.0, pullback=0.0),
           dict(max_paths=16, max_candidates=1)),
    legal_found=_legal_found, untouched=REACH, untouched_found=_untouched_found, yardstick=Mixed,
    empty_world=lambda: World([], ALPHA, TAU, 4, SCAT),
    steady=REACH, fewer=dict(max_paths=16, max_near=32768, max_candidates=2048), steady_found=_steady_found)


@pytest.mark.gpu
def test_errors_and_untouched_state(pkg, oracle_mod):
    contract.errors_and_untouched_state(pkg, oracle_mod, QUERY)


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    contract.steady_state_allocates_nothing(pkg, QUERY)


@pytest.mark.gpu
def test_queries_interleaved_on_one_context(pkg):
    """the six queries share their chain, scan, pair and staging code but no buffer: on one context, in an order in which every
    staging is used (count 5), grown past its first capacity of 32 (count 33) and used again with fewer rows, each call returns the
    bytes it returns as the first call of a fresh context"""
    w = scene_world(2)
    pos = np.random.default_rng(0x2A7E).uniform([50.0, 50.0, 40.0], [440.0, 900.0, 900.0], (33, 3)).astype(np.float32)
    pos[1::2, 0] += np.float32(510.0)
    pos[0] = SRC

    def fresh():
        ctx = w.context(pkg)
        ctx.set_listener(LIS)
        return ctx, place(ctx, pos)

    kinds = ("mixed", "diffraction2", "reflection2", "diffraction", "reflection", "direct")
    calls = [(k, 5) for k in kinds] + [(k, 33) for k in reversed(kinds)] + [(k, 5) for k in kinds]
    got = contract.queries_interleaved_on_one_context(fresh, calls, dict(reflection2=dict(max_length=1e6), diffraction2=dict(max_detour=1000.0),
                                                                         mixed=REACH))
    # the comparison is not of zeros
    by = {c: g for c, g in zip(calls, got)}
    assert by["mixed", 5][0][0]["found"] == 4 and np.any(by["mixed", 33][0]["returned"] > 0)
    assert np.any(by["reflection2", 33][0]["returned"] > 0) and np.any(by["reflection", 33][0]["returned"] > 0)
    assert np.any(by["diffraction", 33][0]["returned"] > 0)


@pytest.mark.gpu
def test_component_layer(pkg, oracle_mod, monkeypatch):
    """a source steps from the lit side to behind the partition: UpdateMixedPaths is Context.mixed_paths over the active sources,
    Voices(mixed=) appends voices whose keys carry the tag no other kind has, and the callback they appear in reports them as
    started; of two paths whose keys collide the earlier stays; without the keyword Voices returns what it returned before"""
    from test_direct_render import noise
    w = scene_world(1)
    frame, taps = 64, 15
    sub = pkg.AudioRayTracingSubsystem(num_bands=4)
    sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
    sub.SetMaterials(w.absorption, w.transmission, w.scattering)
    lit = [250.0, 800.0, 150.0]   # sees the listener past the rim; its reflection behind it passes the rim lit as well
    comp = pkg.FrequenSeeAudioComponent(lit)
    comp.OnRegister(sub)
    sub.SetListenerLocation(LIS)
    plug = pkg.FrequenSeeAudioReflectionPlugin(sub)
    plug.Initialize(frame, taps, 32, 0.05)
    plug.OnInitSource(comp)
    rng = np.random.default_rng(5)
    y = Mixed(oracle_mod, w)
    latency = ((taps - 1) // 2) / sub.ctx.cfg.sample_rate
    seen = []
    for cb, pos in enumerate((lit, lit, SRC, SRC)):
        comp.SetComponentLocation(pos)
        rows, paths = sub.UpdateReflectionPaths(max_paths=8)
        drows, dpaths = sub.UpdateDiffractionPaths()
        mrows, mpaths = got = sub.UpdateMixedPaths(**REACH)
        assert_equal(got, y.expect(pkg, [pos], LIS, **REACH), f"component layer, callback {cb}")
        voices = plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0], diffraction=(drows[0], dpaths[0]), mixed=(mrows[0], mpaths[0]))
        nr, nd, nm = int(rows[0]["returned"]), int(drows[0]["returned"]), int(mrows[0]["returned"])
        assert voices.shape == (nr + nd + nm,)
        if cb >= 2:
            assert nm == 4 and nd >= 1
        assert np.array_equal(voices[:nr + nd], plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0], diffraction=(drows[0], dpaths[0]))), \
            "the other kinds' voices changed"
        out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, right=[0.0, 1.0, 0.0], diffraction=(drows, dpaths),
                                        mixed=(mrows, mpaths))
        assert int(counts[0]["dropped"]) == 0
        for v, p in zip(voices[nr + nd:], mpaths[0][:nm]):
            assert int(v["key"]) == voice_key(p) == plug.MixedKey(p["triangle"], p["edge"], p["end"])
            assert int(v["key"]) >= TAG and np.all(voices["key"][:nr + nd] < TAG)
            assert np.array_equal(v["band_gain"], p["gain"])
            assert float(v["delay"]) == pytest.approx(float(p["delay"]) - latency, abs=1e-7)
            t = (float(np.dot(p["direction"].astype(np.float64), [0.0, 1.0, 0.0])) + 1.0) * np.pi / 4.0
            assert np.allclose(v["channel_gain"], [np.cos(t), np.sin(t)], atol=1e-6)
        seen.append((set(int(k) for k in voices["key"]), {int(k) for k in voices["key"][nr + nd:]}, int(counts[0]["started"])))
    # callback 2 is the one the mixed voices appear in: the callback reports them (and whatever else is new at SRC) as started
    new = seen[2][0] - seen[1][0]
    fresh = seen[2][1] - seen[1][0]
    assert fresh and fresh <= new and len(seen[2][1]) == 4 and seen[2][2] == len(new)
    assert seen[3][2] == 0 and seen[3][0] == seen[2][0], "a steady source starts nothing"
    # a forced collision: all four paths under one key — the first of the row, the shortest, is the one that stays
    monkeypatch.setattr(type(plug), "MixedKey", staticmethod(lambda t, e, end: TAG | 5))
    collided = plug.Voices(rows[0], paths[0], mixed=(mrows[0], mpaths[0]))
    assert collided.shape == (nr + 1,) and int(collided[nr]["key"]) == TAG | 5
    assert np.array_equal(collided[nr]["band_gain"], mpaths[0][0]["gain"]) and mpaths[0][0]["length"] <= mpaths[0][1]["length"]
    out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, mixed=(mrows, mpaths))
    assert int(counts[0]["dropped"]) == 0, "the renderer was handed duplicate keys"
    plug.OnReleaseSource(comp)
    sub.Deinitialize()
