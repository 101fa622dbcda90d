"""fs_update_diffraction2_paths: the diffraction round thick obstacles — two parallel edges — of every source of a tick.

The yardstick is a Python restatement of include/frequensee.h's "second-order diffraction paths" rule on numpy float32, built on the
first-order restatement of tests/test_diffraction_paths.py (its exact fmaf on arrays, its `reached`) and the helpers of
tests/test_reflection_paths.py: the near test as array arithmetic over all edge records, the pair filter per q as array arithmetic
over all near p, the five legs per candidate as scalars round the oracle's brute-force closest hit.  Every field of every row and
path must EQUAL it, floats by bit pattern.  The restatement itself is checked without a GPU against the float64 unfolding of three
half-planes about two parallel lines, length = hypot(dS + g + dL, the distance along the edges), in a shoebox with a thick box whose
apexes are, by assertion, nowhere near a sub-edge's end.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytest.register_assert_rewrite("path_query_contract")
import path_query_contract as contract  # noqa: E402
from path_query_contract import assert_equal  # noqa: E402
from test_diffraction_paths import BLIS, BSRC, Diffraction, fmaf_arrays
from test_diffraction_paths import box_world as corner_box_world
from test_reflection_paths import (ALPHA, HI, LO, NO_MATERIAL, NO_OBJECT, OPAQUE, SCAT, TAU, F, World, bits, box, cross,
                                   dot, fmaf, place, quad_grid, shoebox_world)

DEFAULTS = dict(max_paths=4, max_near=16384, max_candidates=1024, margin=1e-3, max_detour=250.0, min_parallel=0.999, offset=0.1, merge=1.0,
                step=0.1, pullback=0.1, dist_divisor=1000.0, sound_speed=343.0)
OVERFLOW, NEAR_OVERFLOW = 1, 2
TAG = 0x20000000


def voice_key(p):
    kp, kq = 4 * int(p["triangle"][0]) + int(p["edge"][0]), 4 * int(p["triangle"][1]) + int(p["edge"][1])
    return TAG | (((kp * 2654435761 + kq) % 2 ** 32) >> 3)


class Diffraction2(Diffraction):
    """edge record r = 3 i + j of triangle i, edge j (its code in keys and paths is 4 i + j)"""

    def __init__(self, oracle_mod, w, tri=None, edges=None):
        super().__init__(oracle_mod, w, tri, edges)
        v0, e1, e2 = self.v0, self.e1, self.e2
        T = len(v0)
        with np.errstate(all="ignore"):
            n = cross(e1, e2) if T else np.zeros((0, 3), np.float32)
            a = np.stack([v0, v0 + e1, v0 + e2], axis=1).reshape(-1, 3)
            wv = np.stack([e1, e2 - e1, -e2], axis=1).reshape(-1, 3)
            self.rn = np.repeat(n, 3, axis=0)
            self.rnn = dot(self.rn, self.rn) if T else np.zeros(0, np.float32)
            self.rv0 = np.repeat(v0, 3, axis=0)
            self.ra, self.rw = a, wv
            self.rww = dot(wv, wv) if T else np.zeros(0, np.float32)
            self.ro = cross(wv, self.rn) if T else np.zeros((0, 3), np.float32)
            self.roo = dot(self.ro, self.ro) if T else np.zeros(0, np.float32)
        for x in (self.rn, self.ra, self.rw, self.ro, self.rww, self.roo):
            assert x.dtype == np.float32
        self.d2 = dict(short_blocked=0, long_blocked=0, merged=0, pairs=0, parallel=0)

    def near_set(self, S, L, own, max_detour):
        """step 0 over all edge records at once: the near records, ascending"""
        if len(self.ra) == 0:
            return np.zeros(0, np.int64)
        with np.errstate(all="ignore"):
            rS, rL = S[None, :] - self.ra, L[None, :] - self.ra
            reach = np.sqrt(self.rww)
            g = S - L
            bound = np.sqrt(dot(g, g)) + F(max_detour)
            inside = ((np.sqrt(dot(rS, rS)) + np.sqrt(dot(rL, rL))) - (reach + reach)) <= bound
        assert reach.dtype == np.float32 and bound.dtype == np.float32
        is_own = np.array([int(o) != NO_OBJECT and int(o) in own for o in self.w.obj], bool) if own else np.zeros(len(self.v0), bool)
        return np.nonzero((self.rnn != 0) & (self.rww != 0) & (self.roo != 0) & ~np.repeat(is_own, 3) & inside)[0]

    def pairs(self, S, L, near, p):
        """step 1: the ordered pairs (q, p) of near records that pass, each with the values the legs and the row use"""
        out = []
        if len(near) < 2:
            return out
        m, md, mp = F(p["margin"]), F(p["max_detour"]), F(p["min_parallel"])
        mm = F(p["merge"]) * F(p["merge"])
        one = F(1.0)
        with np.errstate(all="ignore"):
            a, w, ww, n, v0, o = self.ra[near], self.rw[near], self.rww[near], self.rn[near], self.rv0[near], self.ro[near]
            rS, rL = S[None, :] - a, L[None, :] - a
            tS, tL = dot(rS, w) / ww, dot(rL, w) / ww
            cS, cL = cross(rS, w), cross(rL, w)
            dS, dL = np.sqrt(dot(cS, cS) / ww), np.sqrt(dot(cL, cL) / ww)
            dt = tL - tS
            dtdS = dt * dS
            hS, hL = dot(S[None, :] - v0, n), dot(L[None, :] - v0, n)
            g3 = S - L
            distance = np.sqrt(dot(g3, g3))
            for jq in range(len(near)):
                aq, wq, wwq, nq, v0q, oq = a[jq], w[jq], ww[jq], n[jq], v0[jq], o[jq]
                c = dot(wq[None, :], w)
                ok = c * c >= mp * (wwq * ww)
                ok[jq] = False
                self.d2["pairs"] += len(near) - 1
                self.d2["parallel"] += int(ok.sum())
                r = a - aq[None, :]
                cg = cross(r, wq[None, :])
                gg = dot(cg, cg)
                ok &= gg > mm * wwq
                i = np.nonzero(ok)[0]   # the rest for the pairs of parallel edges that are not one line only: the same bits, less work
                if len(i) == 0:
                    continue
                ai, wi, wwi, ni, v0i, oi, hLi = a[i], w[i], ww[i], n[i], v0[i], o[i], hL[i]
                g = np.sqrt(gg[i] / wwq)
                dSg = dS[jq] + g
                total = dSg + dL[i]
                t1 = tS[jq] + dtdS[jq] / total
                ok = (total != 0) & (t1 >= -m) & (t1 <= one + m)
                tm = tS[jq] + (dt[jq] * dSg) / total
                E1 = fmaf_arrays(t1[:, None], wq[None, :], aq[None, :])
                P = fmaf_arrays(tm[:, None], wq[None, :], aq[None, :])
                t0 = dot(P - ai, wi) / wwi
                ok &= (t0 >= -m) & (t0 <= one + m)
                E0 = fmaf_arrays(t0[:, None], wi, ai)
                h0 = dot(E0 - v0q[None, :], nq[None, :])
                ok &= ((hS[jq] > 0) & (h0 < 0)) | ((hS[jq] < 0) & (h0 > 0))
                h1 = dot(E1 - v0i, ni)
                ok &= ((hLi > 0) & (h1 < 0)) | ((hLi < 0) & (h1 > 0))
                s1 = hS[jq] / (hS[jq] - h0)
                X1 = fmaf_arrays(s1[:, None], E0 - S[None, :], S[None, :])
                ok &= dot(X1 - E1, oq[None, :]) <= 0
                s0 = h1 / (h1 - hLi)
                X0 = fmaf_arrays(s0[:, None], L[None, :] - E1, E1)
                ok &= dot(X0 - E0, oi) <= 0
                u, mv, v = S[None, :] - E1, E1 - E0, E0 - L[None, :]
                l1, lm, l0 = np.sqrt(dot(u, u)), np.sqrt(dot(mv, mv)), np.sqrt(dot(v, v))
                length = (l1 + lm) + l0
                detour = length - distance
                ok &= (l1 != 0) & (lm != 0) & (l0 != 0) & (detour <= md)
                for x in (E0, E1, g, t0, length, detour):
                    assert x.dtype == np.float32
                for k in np.nonzero(ok)[0]:
                    out.append(dict(q=int(near[jq]), p=int(near[i[k]]), E0=E0[k].copy(), E1=E1[k].copy(), u=u[k].copy(), m=mv[k].copy(),
                                    v=v[k].copy(), l1=l1[k], lm=lm[k], l0=l0[k], length=length[k], detour=detour[k], g=g[k],
                                    hS=hS[jq], hL=hLi[k], t0=t0[k], t1=t1[k]))
        return out

    def ends(self, r, h, E, off):
        """the first-order rule's construction at record r and apex E: (the unit normal towards the end h is measured from, the point
        on that side, the point on the other)"""
        io = F(1.0) / np.sqrt(self.roo[r])
        inn = F(1.0) / np.sqrt(self.rnn[r])
        sg = inn if h > 0 else -inn
        nh = [F(self.rn[r, k] * sg) for k in range(3)]
        Eo = [fmaf(off, F(self.ro[r, k] * io), E[k]) for k in range(3)]
        return nh, [fmaf(off, nh[k], Eo[k]) for k in range(3)], [fmaf(-off, nh[k], Eo[k]) for k in range(3)]

    def long_leg(self, start, end, back, own, step):
        e = np.array([F(end[k] - start[k]) for k in range(3)], np.float32)
        ln = F(np.sqrt(dot(e, e)))
        with np.errstate(all="ignore"):
            inv = F(1.0) / ln
            d = [F(e[k] * inv) for k in range(3)]
        return self.reached(start, d, ln if back is None else F(ln - back), own, step)

    def leg_reached(self, S32, L32, own, c, p, k):
        """leg k = 1 .. 5 of step 2 for candidate c"""
        off = F(p["offset"])
        nq, ES, EM1 = self.ends(c["q"], c["hS"], c["E1"], off)
        np_, EL, EM0 = self.ends(c["p"], c["hL"], c["E0"], off)
        if k == 2:
            return self.reached(ES, [-x for x in nq], F(F(2.0) * off), own, p["step"])
        if k == 4:
            return self.reached(EM0, np_, F(F(2.0) * off), own, p["step"])
        start, end, back = {1: (S32, ES, None), 3: (EM1, EM0, None), 5: (EL, L32, F(p["pullback"]))}[k]
        return self.long_leg(start, end, back, own, p["step"])

    def confirm2(self, S32, L32, own, c, p):
        """step 2: the short legs first, the verdicts are independent"""
        for k in (2, 4, 3, 1, 5):
            if not self.leg_reached(S32, L32, own, c, p, k):
                self.d2["short_blocked" if k in (2, 4) else "long_blocked"] += 1
                return False
        return True

    def code(self, r):
        return 4 * (r // 3) + r % 3

    def row(self, S, L, src_obj=NO_OBJECT, lis_obj=NO_OBJECT, **params):
        """(row dict, the kept paths in the rule's order: all of them, not only max_paths)"""
        p = dict(DEFAULTS, **params)
        S32, L32 = np.array([F(c) for c in S], np.float32), np.array([F(c) for c in L], np.float32)
        own = {i for i in (src_obj, lis_obj) if i != NO_OBJECT}
        zero = dict(near=0, candidates=0, confirmed=0, found=0, returned=0, flags=0)
        near = self.near_set(S32, L32, own, p["max_detour"])
        if len(near) > p["max_near"]:
            return dict(zero, near=len(near), flags=NEAR_OVERFLOW), []
        cand = self.pairs(S32, L32, near, p)
        if len(cand) > p["max_candidates"]:
            return dict(zero, near=len(near), candidates=len(cand), flags=OVERFLOW), []
        conf = [c for c in cand if self.confirm2(list(S32), list(L32), own, c, p)]
        for c in conf:
            c["key"] = (bits(c["length"]), self.code(c["p"]), self.code(c["q"]))
        mm = F(p["merge"]) * F(p["merge"])
        kept = []
        for c in conf:
            if any(d["key"] < c["key"] and dot(c["E0"] - d["E0"], c["E0"] - d["E0"]) < mm and dot(c["E1"] - d["E1"], c["E1"] - d["E1"]) < mm
                   for d in conf):
                self.d2["merged"] += 1
            else:
                kept.append(c)
        kept.sort(key=lambda c: c["key"])
        paths = []
        ss, dd = float(F(p["sound_speed"])), float(F(p["dist_divisor"]))
        for c in kept:
            gain = np.zeros(8, np.float32)
            for b in range(self.B):
                k = F(40.0 * self.f[b] / (ss * dd))
                lam5 = F(5.0 * ss * dd / self.f[b])
                r = lam5 / c["g"]
                rr = r * r
                c3 = (F(1.0) + rr) / ((F(1.0) / F(3.0)) + rr)
                gain[b] = F(1.0) / np.sqrt(F(3.0) + (k * c3) * c["detour"])
            ip, iq = c["p"] // 3, c["q"] // 3
            paths.append(dict(length=c["length"], delay=F(F(c["length"] / F(p["dist_divisor"])) / F(p["sound_speed"])), detour=c["detour"],
                              gap=c["g"], cos_bend=np.array([dot(c["m"], c["v"]) / (c["lm"] * c["l0"]), dot(c["u"], c["m"]) / (c["l1"] * c["lm"])],
                                                            np.float32),
                              apex=np.array([c["E0"], c["E1"]], np.float32), direction=c["v"] * (F(1.0) / c["l0"]),
                              triangle=np.array([ip, iq], np.uint32), edge=np.array([c["p"] % 3, c["q"] % 3], np.uint32),
                              material=np.array([int(self.w.mat[ip]), int(self.w.mat[iq])], np.uint32), gain=gain, t=(c["t0"], c["t1"])))
        return dict(near=len(near), candidates=len(cand), confirmed=len(conf), found=len(kept), returned=min(len(kept), p["max_paths"]),
                    flags=0), paths

    def expect(self, pkg, positions, L, src_obj=None, lis_obj=NO_OBJECT, **params):
        """the call's two arrays as the library must write them"""
        mp = dict(DEFAULTS, **params)["max_paths"]
        rows = np.zeros(len(positions), dtype=pkg.Context.DIFFRACTION2_ROW_DTYPE)
        paths = np.zeros((len(positions), mp), dtype=pkg.Context.DIFFRACTION2_DTYPE)
        for i, S in enumerate(positions):
            r, ps = self.row(S, L, NO_OBJECT if src_obj is None else src_obj[i], lis_obj, **params)
            for k in rows.dtype.names:
                rows[i][k] = r[k]
            for j, y in enumerate(ps[:mp]):
                for k in paths.dtype.names:
                    paths[i, j][k] = y[k]
        return rows, paths


# ---- the scene ------------------------------------------------------------------------------------------------------
SRC, LIS = [300.0, 200.0, 120.0], [720.0, 260.0, 110.0]          # either side of the thick box
BOX = ([450.0, 0.0, 0.0], [550.0, 400.0, 200.0])                 # flush with the y = 0 wall, 100 cm thick, below the ceiling
SIZE = 1000.0
# fp32 against float64: the chain to a length is S - a (1), the dots of tS, tL and ww (5 each), two divides, cS (3 per component), its
# square (5), a divide and a root, the same for dL with its own L - a (11), the gap's a_p - a_q, cross, square, divide and root (11),
# the two sums (2), t1 and tm (3 each), the two fmaf (2), P - a_p, its dot, the divide and the fmaf (8), u, m and v (3), their squares
# (5 each), three roots and two sums — about ninety roundings where test_diffraction_paths.py counts about forty for its 2e-5.
LENGTH_RTOL = 2e-5 * 90 / 40
TOP = dict(length=466.2307, detour=41.849, apex=((550.0, 235.038, 200.0), (450.0, 222.061, 200.0)))
SIDE = dict(length=570.3148, detour=145.933, apex=((550.0, 400.0, 113.862), (450.0, 400.0, 115.616)))


def box_world(n=1, hi=BOX[1], actor=2, extra=()):
    return shoebox_world([(box(BOX[0], hi, n), OPAQUE, actor)] + list(extra), n=n)


def unfold2(S, L, aq, ap, w):
    """float64: (length, E0, E1, g) of the shortest path S -> the line aq + t w -> the parallel line ap + t w -> L"""
    S, L, aq, ap, w = (np.asarray(c, np.float64) for c in (S, L, aq, ap, w))
    lw = np.linalg.norm(w)
    wh = w / lw
    tS, tL = np.dot(S - aq, wh), np.dot(L - aq, wh)
    dS, dL = np.linalg.norm(np.cross(S - aq, wh)), np.linalg.norm(np.cross(L - ap, wh))
    g = np.linalg.norm(np.cross(ap - aq, wh))
    total = dS + g + dL
    E1 = aq + (tS + (tL - tS) * dS / total) * wh
    P = aq + (tS + (tL - tS) * (dS + g) / total) * wh
    E0 = ap + np.dot(P - ap, wh) * wh
    return float(np.hypot(total, tL - tS)), E0, E1, float(g)


def gain64(detour, gap, first_order=False):
    out = []
    for f in (125.0, 250.0, 500.0, 1000.0):
        r = 5.0 * 343.0 * 1000.0 / f / gap
        c3 = 1.0 if first_order else (1.0 + r * r) / (1.0 / 3.0 + r * r)
        out.append(1.0 / np.sqrt(3.0 + 40.0 * f / (343.0 * 1000.0) * c3 * detour))
    return np.array(out)


def check_path(p, ref, S, L):
    length, E0, E1, g = ref
    assert abs(float(p["length"]) - length) <= LENGTH_RTOL * length, (p["length"], length)
    assert np.allclose(p["apex"][0], E0, rtol=0, atol=LENGTH_RTOL * SIZE * 10) and np.allclose(p["apex"][1], E1, rtol=0, atol=LENGTH_RTOL * SIZE * 10)
    # gap is the distance between the two edges' lines (the header's g), the box's thickness: not |E1 - E0|
    assert abs(float(p["gap"]) - 100.0) <= LENGTH_RTOL * 100.0 and abs(g - 100.0) < 1e-9
    straight = float(np.linalg.norm(np.asarray(S, np.float64) - np.asarray(L, np.float64)))
    assert p["detour"] > 0 and abs(float(p["detour"]) - (length - straight)) <= 2 * LENGTH_RTOL * length
    d = (E0 - np.asarray(L, np.float64)) / np.linalg.norm(E0 - np.asarray(L, np.float64))
    assert np.allclose(p["direction"], d, rtol=0, atol=1e-4)
    legs = [E1 - np.asarray(S, np.float64), E0 - E1, np.asarray(L, np.float64) - E0]
    cosines = [np.dot(legs[1], legs[2]) / np.linalg.norm(legs[1]) / np.linalg.norm(legs[2]),
               np.dot(legs[0], legs[1]) / np.linalg.norm(legs[0]) / np.linalg.norm(legs[1])]
    assert np.allclose(p["cos_bend"], cosines, rtol=0, atol=1e-5)
    gn = p["gain"]
    assert np.all(gn[:4] > 0) and np.all(np.diff(gn[:4]) < 0) and np.all(gn[4:] == 0)
    assert np.allclose(gn[:4], gain64(length - straight, 100.0), rtol=1e-4)
    assert np.all(gn[:4] < gain64(length - straight, 100.0, first_order=True)), "C3 > 1"


def references():
    top = unfold2(SRC, LIS, (450.0, 0.0, 200.0), (550.0, 0.0, 200.0), (0.0, 1.0, 0.0))
    side = unfold2(SRC, LIS, (450.0, 400.0, 0.0), (550.0, 400.0, 0.0), (0.0, 0.0, 1.0))
    return top, side


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.Diffraction2Params) == 52 and C.sizeof(cap.Diffraction2Path) == 116 and C.sizeof(cap.Diffraction2Row) == 24
    assert pkg.Context.DIFFRACTION2_DTYPE.itemsize == 116 and pkg.Context.DIFFRACTION2_ROW_DTYPE.itemsize == 24
    P = cap.Diffraction2Path
    names = ("length", "delay", "detour", "gap", "cos_bend", "apex", "direction", "triangle", "edge", "material", "gain")
    offsets = [0, 4, 8, 12, 16, 24, 48, 60, 68, 76, 84]
    assert [getattr(P, k).offset for k in names] == offsets
    assert pkg.Context.DIFFRACTION2_DTYPE.names == names and [pkg.Context.DIFFRACTION2_DTYPE.fields[k][1] for k in names] == offsets
    assert pkg.Context.DIFFRACTION2_ROW_DTYPE.names == ("near", "candidates", "confirmed", "found", "returned", "flags")
    assert [k for k, _ in cap.Diffraction2Row._fields_] == ["near", "candidates", "confirmed", "found", "returned", "flags"]
    p = cap.default_diffraction2_params()
    assert p.struct_size == 52
    assert (p.max_paths, p.max_near, p.max_candidates) == (DEFAULTS["max_paths"], DEFAULTS["max_near"], DEFAULTS["max_candidates"]) == (4, 16384, 1024)
    assert p.margin == F(1e-3) and p.offset == F(0.1) and p.step == F(0.1) and p.pullback == F(0.1) and p.min_parallel == F(0.999)
    assert p.max_detour == F(DEFAULTS["max_detour"]) and p.merge == 1.0 and p.dist_divisor == 1000.0 and p.sound_speed == 343.0
    assert (cap.MAX_DIFFRACTION2_PATHS, cap.MAX_DIFFRACTION2_NEAR, cap.MAX_DIFFRACTION2_CANDIDATES, cap.MAX_DIFFRACTION2_BATCH,
            cap.DIFFRACTION2_OVERFLOW, cap.DIFFRACTION2_NEAR_OVERFLOW, cap.DIFFRACTION2_VOICE_TAG) == (16, 32768, 2048, 256, 1, 2, TAG)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frequensee.h")).read()
    for name, value in (("FS_MAX_DIFFRACTION2_PATHS", "16"), ("FS_MAX_DIFFRACTION2_NEAR", "32768"), ("FS_MAX_DIFFRACTION2_CANDIDATES", "2048"),
                        ("FS_MAX_DIFFRACTION2_BATCH", "256"), ("FS_DIFFRACTION2_OVERFLOW", "1u"), ("FS_DIFFRACTION2_NEAR_OVERFLOW", "2u")):
        assert f"#define {name}" in header and header.split(f"#define {name}")[1].split()[0] == value
    assert cap.load().fs_abi_version() == 5, "the change only adds"
    # the four kinds of voice keys are disjoint ranges
    assert TAG == cap.REFLECTION2_VOICE_TAG >> 1 == cap.DIFFRACTION_VOICE_TAG >> 2
    assert TAG <= voice_key(dict(triangle=[2 ** 29 - 1, 2 ** 29 - 1], edge=[2, 2])) < cap.REFLECTION2_VOICE_TAG


def test_exported_in_one_tier(pkg):
    contract.exported_in_one_tier(pkg, ("fs_diffraction2_params_default", "fs_update_diffraction2_paths"))


def test_null_context_and_no_device(pkg):
    contract.null_context_and_no_device(pkg, QUERY)


def test_reference_figures():
    top, side = references()
    straight = float(np.linalg.norm(np.asarray(SRC) - np.asarray(LIS)))
    assert abs(straight - 424.3819) < 5e-4
    for ref, want in ((top, TOP), (side, SIDE)):
        assert abs(ref[0] - want["length"]) < 5e-4 and abs(ref[0] - straight - want["detour"]) < 5e-3
        assert np.allclose(ref[1], want["apex"][0], atol=5e-3) and np.allclose(ref[2], want["apex"][1], atol=5e-3)
    for n in (1, 2, 4):   # (on the input) no apex near the end of a sub-edge
        for ref, axis, extent in ((top, 1, 400.0), (side, 2, 200.0)):
            for apex in ref[1:3]:
                t = apex[axis] / (extent / n)
                assert min(t - np.floor(t), np.ceil(t) - t) > 0.02


@pytest.mark.parametrize("n", [1, 2, 4])
def test_restatement_thick_box(pkg, oracle_mod, n):
    """over the top and round the free side of a box that no first-order path gets round"""
    top, side = references()
    w = box_world(n)
    assert len(w.tri) == 24 * n * n
    y = Diffraction2(oracle_mod, w)
    first_order, _ = Diffraction.row(y, SRC, LIS)
    assert first_order["found"] == 0, "the gap this query closes"
    r, paths = y.row(SRC, LIS)
    assert r["near"] == {1: 68, 2: 250, 4: 864}[n] and r["flags"] == 0   # (of 72 n n: the bound is an ellipsoid, the far corners are out)
    assert r["confirmed"] >= r["found"] == r["returned"] == 2 == len(paths), r
    assert r["candidates"] > r["confirmed"]
    if n > 1:
        assert y.d2["short_blocked"] > 0
    check_path(paths[0], top, SRC, LIS)
    check_path(paths[1], side, SRC, LIS)
    for p in paths:
        assert all(min(t - np.floor(t), np.ceil(t) - t) > 0.02 for t in p["t"])
    first = 12 * n * n   # the box's triangles follow the room's; its walls x lo and x hi are the first two
    assert all(p["triangle"][0] // (2 * n * n) - 6 == 1 and p["triangle"][1] // (2 * n * n) - 6 == 0 for p in paths), "p on x hi, q on x lo"
    assert all(np.all(p["triangle"] >= first) for p in paths)
    assert paths[0]["length"] < paths[1]["length"] and np.all(paths[0]["gain"][:4] > paths[1]["gain"][:4])
    assert len({voice_key(p) for p in paths}) == 2
    # min_parallel = 1: the axis-aligned rims are exactly parallel
    r1, paths1 = y.row(SRC, LIS, min_parallel=1.0)
    assert r1["found"] == 2 and [bits(p["length"]) for p in paths1] == [bits(p["length"]) for p in paths]


def test_restatement_lit_listener_and_one_corner(pkg, oracle_mod):
    w = box_world(2)
    y = Diffraction2(oracle_mod, w)
    lit = [300.0, 600.0, 110.0]   # past the box's free side: the segment to SRC is free
    e = np.asarray(lit, np.float32) - np.asarray(SRC, np.float32)
    ln = F(np.sqrt(dot(e, e)))
    assert y.leg([F(c) for c in SRC], [F(c / ln) for c in e], ln, set(), -1, 0.1)[0] == 0   # FREE
    r, paths = y.row(SRC, lit)
    assert r["found"] == 0 and not paths
    # both ends see one corner of the first-order tests' box: the shadow test at the listener's end rejects every pair
    y = Diffraction2(oracle_mod, corner_box_world(2))
    r, paths = y.row(BSRC, BLIS)
    assert r["found"] == 0 and r["near"] > 0
    assert Diffraction.row(y, BSRC, BLIS)[0]["found"] == 1, "the first-order query still finds its one path"


def test_restatement_both_gaps(pkg, oracle_mod):
    """a box 0.5 cm thick: every pair of its rims is within merge — the first-order query's business; a sheet: no second rim"""
    thin = shoebox_world([(box([450.0, 0.0, 0.0], [450.5, 400.0, 200.0]), OPAQUE, 2)])
    y = Diffraction2(oracle_mod, thin)
    r, _ = y.row(SRC, LIS)
    S32, L32 = np.asarray(SRC, np.float32), np.asarray(LIS, np.float32)
    cand = y.pairs(S32, L32, y.near_set(S32, L32, set(), DEFAULTS["max_detour"]), DEFAULTS)
    # no two rims 0.5 cm apart are a candidate; what the filter leaves pairs a rim with the opposite rim of the other face, a gap of a
    # whole face, and runs through the box: the legs reject it
    assert r["near"] == 68 and r["candidates"] == len(cand) and all(c["g"] > 100.0 for c in cand) and r["confirmed"] == r["found"] == 0, r
    assert y.row(SRC, LIS, merge=0.25)[0]["found"] == 2, "the same box with merge below its thickness"
    sheet = shoebox_world([(quad_grid((500.0, 0.0, 0.0), (0.0, 400.0, 0.0), (0.0, 0.0, 200.0), 1), OPAQUE, 2)])
    y = Diffraction2(oracle_mod, sheet)
    r, _ = y.row(SRC, LIS)
    assert r["candidates"] == 0 and r["found"] == 0
    assert Diffraction.row(y, SRC, LIS)[0]["found"] == 2


def rotated_box_world(degrees=17.0):
    """the box turned about the vertical through (500, 200): its fp32 rims are parallel only up to rounding"""
    t = np.deg2rad(degrees)
    b = box([450.0, 100.0, 0.0], [550.0, 400.0, 200.0]).astype(np.float64)
    x, yy = b[..., 0] - 500.0, b[..., 1] - 250.0
    b[..., 0], b[..., 1] = 500.0 + np.cos(t) * x - np.sin(t) * yy, 250.0 + np.sin(t) * x + np.cos(t) * yy
    return shoebox_world([(b.astype(np.float32), OPAQUE, 2)])


def test_restatement_rotated_box(pkg, oracle_mod):
    """free on both sides, so three ways round: over the top and round either side; the default min_parallel takes fp32 rims that are
    not exactly parallel"""
    w = rotated_box_world()
    y = Diffraction2(oracle_mod, w)
    rims = w.tri[12:16]   # its walls x lo: the vertical and the top edges of the turned face
    e = (rims[:, 1] - rims[:, 0]).astype(np.float64)
    assert np.any((np.abs(e[:, 0]) > 0) & (np.abs(e[:, 1]) > 0)), "the face is not turned"
    r, paths = y.row(SRC, LIS)
    assert r["found"] == 3 and r["flags"] == 0, r
    assert sorted(int(round(float(p["apex"][0][2]))) == 200 for p in paths) == [False, False, True], "one over the top, two round the sides"
    for p in paths:
        assert abs(float(p["gap"]) - 100.0) < 1e-2


# ---- GPU ---------------------------------------------------------------------------------------------------------------
check = contract.checker("diffraction2")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4], ids=["68_near_records", "864_near_records"])
def test_thick_box(pkg, oracle_mod, n):
    """n = 1: one workgroup of q, one partly full tile of p; n = 4: four workgroups of q and four tiles of p, the last partly full"""
    w = box_world(n)
    assert 3 * len(w.tri) == 72 * n * n
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, paths = check(pkg, ctx, Diffraction2(oracle_mod, w), h, [SRC], LIS, f"thick box n={n}")
    assert rows[0]["near"] == {1: 68, 4: 864}[n] and tuple(rows[0])[3:] == (2, 2, 0) and rows[0]["confirmed"] >= 2
    assert np.all(paths[0][2:].view(np.uint8) == 0)
    assert ctx.diffraction_paths(h)[0][0]["found"] == 0, "the first-order query finds nothing here"
    check(pkg, ctx, Diffraction2(oracle_mod, w), h, [SRC], LIS, f"thick box n={n}, min_parallel 1", min_parallel=1.0)
    ctx.close()


# ---- near lists that end at the edges of the pair kernel's tiles ---------------------------------------------------------
# The pair kernel streams a row's near list through LDS in tiles of 256 entries, shared among at most 16 workgroups per tile of q:
# a list of 255, 256 and 257 entries ends one entry either side of a tile's edge, one of 4100 has 17 tiles (one workgroup takes two).
TILE_EDGE_NEAR = (255, 256, 257, 4100)
_tile_edges = {}


def sparse_field(count):
    """count triangles of 1 cm, 11 cm apart above the thick box, each turned a little further about z: their edges are parallel to
    no rim, so the paths stay the thick box's"""
    k = np.arange(count)
    v0 = np.stack([250.0 + 11.0 * (k % 48), 20.0 + 11.0 * (k // 48), np.full(count, 260.0)], axis=1)
    a = 0.3 + 0.9 * k / max(count, 1)
    e1 = np.stack([np.cos(a), np.sin(a), np.zeros(count)], axis=1)
    e2 = np.stack([-np.sin(a), np.cos(a), np.zeros(count)], axis=1)
    return np.stack([v0, v0 + e1, v0 + e2], axis=1).astype(np.float32)


def tile_edge_case(pkg, oracle_mod, near):
    """(world, max_detour, the call's two arrays by the restatement): the thick box with a sparse field of more edge records than
    asked for, and the max_detour that lies between the near bounds of record number `near` and the next — computed once"""
    if near not in _tile_edges:
        w = box_world(extra=[(sparse_field(near // 3 + 24), OPAQUE, 3)])
        y = Diffraction2(oracle_mod, w)
        S32, L32 = np.asarray(SRC, np.float32), np.asarray(LIS, np.float32)
        with np.errstate(all="ignore"):
            rS, rL, reach, g = S32[None, :] - y.ra, L32[None, :] - y.ra, np.sqrt(y.rww), S32 - L32
            need = np.sort(((np.sqrt(dot(rS, rS)) + np.sqrt(dot(rL, rL))) - (reach + reach)) - np.sqrt(dot(g, g)))
        assert need.dtype == np.float32 and len(need) > near and need[near] - need[near - 1] > 1e-2, "no max_detour cuts the list there"
        detour = float(need[near - 1]) + 0.5 * float(need[near] - need[near - 1])
        assert detour > TOP["detour"] + 1.0
        _tile_edges[near] = w, detour, y.expect(pkg, [SRC], LIS, max_detour=detour)
    return _tile_edges[near]


@pytest.mark.parametrize("near", TILE_EDGE_NEAR)
def test_tile_edge_preconditions(pkg, oracle_mod, near):
    """the restatement alone: the near list has the length asked for, the candidates stay a handful and paths are found"""
    rows, paths = tile_edge_case(pkg, oracle_mod, near)[2]
    assert rows[0]["near"] == near and 0 < rows[0]["candidates"] <= 64 and rows[0]["returned"] > 0 and rows[0]["flags"] == 0
    assert np.all(paths[0]["length"][:rows[0]["returned"]] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("near", TILE_EDGE_NEAR)
def test_near_list_at_tile_edges(pkg, oracle_mod, near):
    w, detour, want = tile_edge_case(pkg, oracle_mod, near)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    got = ctx.diffraction2_paths(place(ctx, [SRC]), max_detour=detour)
    assert_equal(got, want, f"near list of {near}")
    assert got[0][0]["near"] == near and got[0][0]["returned"] > 0
    ctx.close()


BLOCKERS = {   # a small quad across each leg of the path over the top (apexes at y = 222 and 235, z = 200)
    "leg 1": quad_grid((400.0, 150.0, 150.0), (0.0, 150.0, 0.0), (0.0, 0.0, 60.0), 1),       # between S and the near rim, across x = 400
    "leg 2": quad_grid((449.95, 210.0, 200.05), (0.0, 30.0, 0.0), (0.0, 0.0, 10.0), 1),       # a lip standing on the near rim, off the face
    "leg 3": quad_grid((500.0, 200.0, 200.0), (0.0, 60.0, 0.0), (0.0, 0.0, 30.0), 1),         # a fin on the top face
    "leg 4": quad_grid((550.05, 220.0, 200.05), (0.0, 30.0, 0.0), (0.0, 0.0, 10.0), 1),       # a lip standing on the far rim
    "leg 5": quad_grid((640.0, 200.0, 120.0), (0.0, 100.0, 0.0), (0.0, 0.0, 80.0), 1),        # between the far rim and L
}


def over_the_top(p):
    return abs(float(p["apex"][0][0]) - 550.0) < 1e-3 and abs(float(p["apex"][1][0]) - 450.0) < 1e-3 and \
        abs(float(p["apex"][0][2]) - 200.0) < 1e-3 and abs(float(p["apex"][1][2]) - 200.0) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("leg", sorted(BLOCKERS))
def test_each_leg_blocked(pkg, oracle_mod, leg):
    w = box_world(1, extra=[(BLOCKERS[leg], OPAQUE, 3)])
    y = Diffraction2(oracle_mod, w)
    # (on the restatement) the pair over the top is still a candidate, and of its five legs the one meant is blocked and no other
    S32, L32 = np.asarray(SRC, np.float32), np.asarray(LIS, np.float32)
    top = [c for c in y.pairs(S32, L32, y.near_set(S32, L32, set(), DEFAULTS["max_detour"]), DEFAULTS) if over_the_top(dict(apex=[c["E0"], c["E1"]]))]
    assert len(top) == 1
    assert [k for k in range(1, 6) if not y.leg_reached(list(S32), list(L32), set(), top[0], DEFAULTS, k)] == [int(leg[-1])]
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, y, place(ctx, [SRC]), [SRC], LIS, leg)
    got = paths[0][:rows[0]["returned"]]
    assert not any(over_the_top(p) for p in got), "the path over the top survived its blocker"
    assert any(abs(float(p["apex"][0][1]) - 400.0) < 1e-3 for p in got), "the path round the side is untouched"
    ctx.close()


@pytest.mark.gpu
def test_box_to_the_ceiling_and_own_actor(pkg, oracle_mod):
    w = box_world(2, hi=[550.0, 400.0, 300.0])
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Diffraction2(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, "to the ceiling")
    assert tuple(rows[0])[3:] == (1, 1, 0) and abs(float(paths[0][0]["apex"][0][1]) - 400.0) < 1e-3, "only round the side"
    ctx.close()
    # the box as the source's own actor: its records are never near and the legs pass through it; under a foreign id: both paths
    w = box_world(1, actor=8)
    y = Diffraction2(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, _ = check(pkg, ctx, y, h, [SRC], LIS, "foreign id")
    assert rows[0]["near"] == 68 and tuple(rows[0])[3:] == (2, 2, 0)
    ctx.set_source_object(h[0], 8)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "own actor", src_obj=[8])
    assert tuple(rows[0]) == (32, 0, 0, 0, 0, 0) and np.all(paths.view(np.uint8) == 0)
    ctx.set_source_object(h[0], NO_OBJECT)
    ctx.set_listener_object(8)
    rows, _ = check(pkg, ctx, y, h, [SRC], LIS, "the listener's actor", lis_obj=8)
    assert tuple(rows[0]) == (32, 0, 0, 0, 0, 0)
    ctx.close()


@pytest.mark.gpu
def test_caps(pkg, oracle_mod):
    w = box_world(2)
    y = Diffraction2(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    full = ctx.diffraction2_paths(h)
    near, cands, confirmed = (int(full[0][0][k]) for k in ("near", "candidates", "confirmed"))
    assert near == 250 and cands > confirmed >= 2 and tuple(full[0][0])[3:] == (2, 2, 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "near exactly at the cap", max_near=near)
    assert rows.tobytes() == full[0].tobytes() and paths.tobytes() == full[1].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "near overflow", max_near=near - 1)
    assert tuple(rows[0]) == (near, 0, 0, 0, 0, NEAR_OVERFLOW) and np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "candidates exactly at the cap", max_candidates=cands, max_paths=16)
    assert tuple(rows[0]) == tuple(full[0][0]) and paths.shape == (1, 16) and np.all(paths[0][2:].view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "candidate overflow", max_candidates=cands - 1)
    assert tuple(rows[0]) == (near, cands, 0, 0, 0, OVERFLOW) and np.all(paths.view(np.uint8) == 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "paths exactly at the cap", max_paths=2)
    assert tuple(rows[0]) == tuple(full[0][0]) and paths.tobytes() == full[1][0][:2].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "the shortest", max_paths=1)
    assert tuple(rows[0])[3:] == (2, 1, 0) and paths.shape == (1, 1) and paths[0].tobytes() == full[1][0][:1].tobytes()
    # max_detour just above and just below the top path's detour: it is in, then out; the longer path round the side is out both times
    detour = float(full[1][0][0]["detour"])
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "detour cap above", max_detour=detour * (1.0 + 1e-5))
    assert rows[0]["found"] == 1 and paths[0][0].tobytes() == full[1][0][0].tobytes() and rows[0]["near"] < near
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "detour cap below", max_detour=detour * (1.0 - 1e-5))
    assert rows[0]["found"] == 0
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "merge 0", merge=0.0)
    assert rows[0]["found"] >= 2 and rows[0]["found"] == rows[0]["confirmed"]
    ctx.close()


@pytest.mark.gpu
def test_materials_degenerate_triangles_and_bands(pkg, oracle_mod):
    room = box(LO, HI)
    b = box(BOX[0], BOX[1])
    degenerate = np.array([[[450.0, 100.0, 250.0], [450.0, 100.0, 250.0], [450.0, 300.0, 260.0]],      # two corners equal
                           [[550.0, 0.0, 210.0], [550.0, 200.0, 230.0], [550.0, 400.0, 250.0]],        # three on a line
                           [[500.0, 300.0, 220.0], [500.0, 300.0, 220.0], [500.0, 300.0, 220.0]]], np.float32)   # a point
    # the box's walls x lo: no material; x hi: an id beyond the table; the rest: material 0; three bands
    w = World([(room, 0, 1), (b[0:2], NO_MATERIAL, 2), (b[2:4], 9, 2), (b[4:12], 0, 2), (degenerate, 0, 2)],
              [a[:3] for a in ALPHA], [t[:3] for t in TAU], 3, [x[:3] for x in SCAT])
    y = Diffraction2(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "materials")
    assert rows[0]["near"] == 68 and tuple(rows[0])[3:] == (2, 2, 0), "a degenerate triangle was near"
    for p in paths[0][:2]:
        assert tuple(int(m) for m in p["material"]) == (9, NO_MATERIAL) and np.all(p["gain"][:3] > 0) and np.all(p["gain"][3:] == 0)
    for k in ("length", "delay", "detour", "gap", "cos_bend", "apex", "direction", "gain"):
        assert np.all(np.isfinite(paths[k]))
    edges = [300.0, 1200.0]
    ctx.set_band_edges(edges)
    check(pkg, ctx, Diffraction2(oracle_mod, w, edges=edges), h, [SRC], LIS, "edges given")
    ctx.set_band_edges(None)
    check(pkg, ctx, y, h, [SRC], LIS, "default edges again")
    ctx.close()
    one = World([(room, 0, 1), (b, 0, 2)], [[0.5]], [[0.0]], 1, [[0.5]])
    ctx = one.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Diffraction2(oracle_mod, one), place(ctx, [SRC]), [SRC], LIS, "one band")
    assert rows[0]["found"] == 2 and np.all(paths[0]["gain"][:2, 0] > 0) and np.all(paths[0]["gain"][:, 1:] == 0)
    ctx.close()


ROOMS_DETOUR = 150.0
_rooms = {}


def rooms_case(pkg, oracle_mod):
    """starter_room, 8 of its seeded sources — chosen on the CPU, by running the restatement's filters over the first of them, so that
    every row has at most 2000 near records, six have candidates and two a path (test_rooms asserts what matters of that) — and
    the restatement's arrays, computed once"""
    if not _rooms:
        sc = pkg.scenes.starter_room(4)
        tr, sca = pkg.scenes.material_lobes(sc)
        w = World([], sc.absorption, tr, 4, sca)
        w.tri, w.mat, w.obj = sc.triangles.astype(np.float32), sc.material_ids.astype(np.uint16), sc.object_ids.astype(np.uint32)
        y = Diffraction2(oracle_mod, w)
        lo, hi = w.tri.reshape(-1, 3).min(axis=0), w.tri.reshape(-1, 3).max(axis=0)
        pos = np.random.default_rng(0xD2FF).uniform(lo, hi, (256, 3)).astype(np.float32)[[5, 10, 11, 13, 19, 20, 21, 23]]
        _rooms.update(w=w, pos=pos, lis=sc.listener, want=y.expect(pkg, pos, sc.listener, max_detour=ROOMS_DETOUR))
    return _rooms


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["sah", "device_morton"])
def test_rooms(pkg, oracle_mod, fast):
    rc = rooms_case(pkg, oracle_mod)
    wrows = rc["want"][0]
    assert np.all(wrows["near"] <= 2000) and not np.any(wrows["flags"]) and np.any(wrows["returned"] > 0), wrows
    assert np.any(wrows["near"] > 4 * 256) and np.any(wrows["confirmed"] < wrows["candidates"])   # the case is not trivial
    ctx = rc["w"].context(pkg, fast=fast)
    ctx.set_listener(rc["lis"])
    h = place(ctx, rc["pos"])
    rows, paths = got = ctx.diffraction2_paths(h, max_detour=ROOMS_DETOUR)
    assert_equal(got, rc["want"], f"rooms fast={fast}")
    contract.batch_agrees(ctx.diffraction2_paths, h, got, singles=not fast, max_detour=ROOMS_DETOUR)
    ctx.close()


@pytest.mark.gpu
def test_mover(pkg, oracle_mod):
    """the box to the ceiling with a door as thick as it that shuts the gap beside it: no path; the door slid out of the room: the
    path round the box's side; the door back: none"""
    door = box([450.0, 400.0, 0.0], [550.0, 800.0, 300.0])
    w = box_world(1, hi=[550.0, 400.0, 300.0], extra=[(door, OPAQUE, 5)])
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, _ = check(pkg, ctx, Diffraction2(oracle_mod, w), h, [SRC], LIS, "door shut")
    assert rows[0]["found"] == 0
    aside = np.array([[1, 0, 0, 0], [0, 1, 0, 500], [0, 0, 1, 0]], np.float32)
    ctx.set_object_transforms([5], aside[None])
    rows, paths = check(pkg, ctx, Diffraction2(oracle_mod, w, contract.transformed(w, 5, aside)), h, [SRC], LIS, "door aside, no explicit refit")   # the call refits first
    assert rows[0]["found"] == 1 and abs(float(paths[0][0]["apex"][0][1]) - 400.0) < 1e-3
    ctx.set_object_transforms([5], np.eye(3, 4, dtype=np.float32)[None])
    rows, _ = check(pkg, ctx, Diffraction2(oracle_mod, w), h, [SRC], LIS, "door back")
    assert rows[0]["found"] == 0
    ctx.close()


def _defaults_found(t, oracle_mod, want):
    assert_equal(want, Diffraction2(oracle_mod, t.w).expect(t.pkg, [SRC, SRC], LIS), "defaults, one handle twice")
    assert tuple(want[0][0])[3:] == (2, 2, 0)


def _legal_found(rows):
    assert tuple(rows[0])[2:] == (0, 0, 0, OVERFLOW) and rows[0]["candidates"] > 1


def _steady_found(ctx, h, first, fewer):
    assert np.all(first[0]["found"] == 2)


inf, nan = float("inf"), float("nan")
QUERY = contract.Query(
    kind="diffraction2", dtypes=("DIFFRACTION2_ROW_DTYPE", "DIFFRACTION2_DTYPE"), world=lambda: box_world(1), src=SRC, lis=LIS, wrong_struct_size=44,
    null_paths=4, refused_without_device=(dict(max_detour=0.0), dict(min_parallel=0.0), dict(min_parallel=1.5), dict(max_near=0)),
    refused=(dict(max_paths=0), dict(max_paths=17), dict(max_near=0), dict(max_near=32769), dict(max_candidates=0), dict(max_candidates=2049),
             dict(margin=-1e-3), dict(margin=nan), dict(margin=inf), dict(max_detour=0.0), dict(max_detour=-1.0), dict(max_detour=nan),
             dict(max_detour=inf), dict(min_parallel=0.0), dict(min_parallel=-0.5), dict(min_parallel=1.0001), dict(min_parallel=nan),
             dict(min_parallel=inf), dict(offset=-0.1), dict(offset=nan), dict(offset=inf), dict(merge=-1.0), dict(merge=nan), dict(merge=inf),
             dict(step=-0.1), dict(step=nan), dict(step=inf), dict(pullback=-1.0), dict(pullback=nan), dict(pullback=inf),
             dict(dist_divisor=0.0), dict(dist_divisor=-1.0), dict(dist_divisor=nan), dict(dist_divisor=inf), dict(sound_speed=0.0),
             dict(sound_speed=-1.0), dict(sound_speed=nan), dict(sound_speed=inf)),
    defaults_found=_defaults_found,
    legal=(dict(max_paths=16, max_near=32768, max_candidates=2048, margin=0.0, min_parallel=1.0, offset=0.0, merge=0.0, step=0.0, pullback=0.0),
           dict(max_paths=16, max_candidates=1)),
    legal_found=_legal_found, yardstick=Diffraction2, empty_world=lambda: World([], ALPHA, TAU, 4, SCAT),
    fewer=dict(max_paths=16, max_near=32768, max_candidates=2048), steady_found=_steady_found)


@pytest.mark.gpu
def test_errors_and_untouched_state(pkg, oracle_mod):
    contract.errors_and_untouched_state(pkg, oracle_mod, QUERY)


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    contract.steady_state_allocates_nothing(pkg, QUERY)


def interleaved_positions():
    """33 seeded positions, the even ones on SRC's side of the box and the odd ones on the listener's"""
    pos = np.random.default_rng(0x2A7E).uniform([50.0, 50.0, 40.0], [440.0, 750.0, 260.0], (33, 3)).astype(np.float32)
    pos[1::2, 0] += np.float32(510.0)
    pos[0] = SRC
    return pos


@pytest.mark.gpu
def test_queries_interleaved_on_one_context(pkg):
    """the five queries share their chain, scan and staging code but no buffer: on one context, in an order in which every staging is
    used (count 5), grown past its first capacity of 32 (count 33) and used again with fewer rows, each call returns the bytes it
    returns as the first call of a fresh context"""
    w = box_world(2)
    pos = interleaved_positions()

    def fresh():
        ctx = w.context(pkg)
        ctx.set_listener(LIS)
        return ctx, place(ctx, pos)

    calls = [("diffraction2", 5), ("reflection2", 5), ("diffraction", 5), ("direct", 33), ("reflection", 5), ("diffraction2", 33), ("reflection2", 33),
             ("diffraction", 33), ("reflection", 33), ("direct", 5), ("diffraction2", 5), ("reflection2", 5), ("diffraction", 5), ("reflection", 5)]
    got = contract.queries_interleaved_on_one_context(fresh, calls, dict(reflection2=dict(max_length=1e6)))
    # the comparison is not of zeros
    assert np.any(got[5][0]["returned"] > 0) and np.any(got[6][0]["returned"] > 0) and np.any(got[8][0]["returned"] > 0)
    assert got[0][0][0]["found"] == 2


@pytest.mark.gpu
def test_component_layer(pkg, oracle_mod, monkeypatch):
    """a source steps from the lit side to behind the box: UpdateDiffraction2Paths is Context.diffraction2_paths over the active
    sources, Voices(diffraction2=) appends voices whose keys carry the tag no other kind has, and the callback they appear in reports
    them as started; of two paths whose keys collide the earlier stays; without the keyword Voices returns what it returned before"""
    from test_direct_render import noise
    w = box_world(1)
    frame, taps = 64, 15
    sub = pkg.AudioRayTracingSubsystem(num_bands=4)
    sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
    sub.SetMaterials(w.absorption, w.transmission, w.scattering)
    lit = [300.0, 600.0, 120.0]   # sees the listener past the box's free side
    comp = pkg.FrequenSeeAudioComponent(lit)
    comp.OnRegister(sub)
    sub.SetListenerLocation(LIS)
    plug = pkg.FrequenSeeAudioReflectionPlugin(sub)
    plug.Initialize(frame, taps, 32, 0.05)
    plug.OnInitSource(comp)
    rng = np.random.default_rng(5)
    y = Diffraction2(oracle_mod, w)
    latency = ((taps - 1) // 2) / sub.ctx.cfg.sample_rate
    seen = []
    for cb, pos in enumerate((lit, lit, SRC, SRC)):
        comp.SetComponentLocation(pos)
        rows, paths = sub.UpdateReflectionPaths(max_paths=8)
        drows, dpaths = got = sub.UpdateDiffraction2Paths()
        assert_equal(got, y.expect(pkg, [pos], LIS), f"component layer, callback {cb}")
        voices = plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0], diffraction2=(drows[0], dpaths[0]))
        nr, nd = int(rows[0]["returned"]), int(drows[0]["returned"])
        assert voices.shape == (nr + nd,) and nd == (2 if cb >= 2 else 0)
        assert np.array_equal(voices[:nr], plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0])), "the reflections' voices changed"
        out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, right=[0.0, 1.0, 0.0], diffraction2=(drows, dpaths))
        assert int(counts[0]["dropped"]) == 0
        for v, p in zip(voices[nr:], dpaths[0][:nd]):
            assert int(v["key"]) == voice_key(p) == plug.Diffraction2Key(p["triangle"], p["edge"])
            assert TAG <= int(v["key"]) < 0x40000000 and np.all(voices["key"][:nr] < TAG)
            assert np.array_equal(v["band_gain"], p["gain"])
            assert float(v["delay"]) == pytest.approx(float(p["delay"]) - latency, abs=1e-7)
        seen.append((set(int(k) for k in voices["key"]), {int(k) for k in voices["key"][nr:]}, int(counts[0]["started"])))
    # callback 2 is the one the bent voices appear in: the callback reports them (and any reflection new at SRC) as started
    new = seen[2][0] - seen[1][0]
    assert seen[2][1] <= new and len(seen[2][1]) == 2 and seen[2][2] == len(new)
    assert seen[3][2] == 0 and seen[3][0] == seen[2][0], "a steady source starts nothing"
    # a forced collision: both paths under one key — the first of the row, the shorter, is the one that stays
    monkeypatch.setattr(type(plug), "Diffraction2Key", staticmethod(lambda t, e: TAG | 5))
    collided = plug.Voices(rows[0], paths[0], diffraction2=(drows[0], dpaths[0]))
    assert collided.shape == (nr + 1,) and int(collided[nr]["key"]) == TAG | 5
    assert np.array_equal(collided[nr]["band_gain"], dpaths[0][0]["gain"]) and dpaths[0][0]["length"] < dpaths[0][1]["length"]
    out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, diffraction2=(drows, dpaths))
    assert int(counts[0]["dropped"]) == 0, "the renderer was handed duplicate keys"
    plug.OnReleaseSource(comp)
    sub.Deinitialize()
