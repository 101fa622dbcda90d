"""fs_update_diffraction_paths: the first-order edge diffraction of every source of a tick.

The yardstick is a Python restatement of include/frequensee.h's "diffraction paths" rule on numpy float32 (every operation rounded
on its own, fmaf exact): the filter over all (triangle, edge) as float32 array arithmetic, the three legs per candidate as scalars
round oracle.Scene.trace_closest(brute=True) — the scan tests/test_gpu_parity.py holds the GPU line trace to bit for bit — the
records from the test's own vertices, the pass-through rule from the test's own object ids, k_b from the test's own band centres.
Every field of every row and path must EQUAL it, floats by bit pattern.  The restatement itself is checked without a GPU against the
float64 closed form (unfold the two half-planes that meet in the edge: length = hypot(dS + dL, the distance along the edge)) in a
shoebox with a single-sheet partition and with a thick box, at apexes that are, by assertion, nowhere near a sub-edge's end.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytest.register_assert_rewrite("path_query_contract")
import path_query_contract as contract  # noqa: E402
from path_query_contract import assert_equal  # noqa: E402
from test_reflection_paths import (ALPHA, F, FREE, HI, LO, NO_MATERIAL, NO_OBJECT, OPAQUE, SCAT, TAU, Restatement, World, bits, box, cross,
                                   dot, fmaf, place, quad_grid, shoebox_world)

DEFAULTS = dict(max_paths=4, max_candidates=1024, margin=1e-3, max_detour=1000.0, offset=0.1, merge=1.0, step=0.1, pullback=0.1,
                dist_divisor=1000.0, sound_speed=343.0)


def fmaf_arrays(a, b, c):
    """test_reflection_paths.fmaf on float32 arrays: the exact product in double, the sum rounded to odd, one rounding to float32"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = (err != 0) & np.isfinite(s) & np.isfinite(err) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def band_centres(B, edges=None):
    """f_b of the header, in double like the host: sqrt(lo hi), the outer bands an octave wide"""
    e = [125.0 * 2.0 ** (b - 0.5) for b in range(1, B)] if edges is None else [float(x) for x in edges]
    if B == 1:
        return [1000.0]
    return [float(np.sqrt((e[0] / 2.0 if b == 0 else e[b - 1]) * (e[B - 2] * 2.0 if b == B - 1 else e[b]))) for b in range(B)]


class Diffraction(Restatement):
    def __init__(self, oracle_mod, w, tri=None, edges=None):
        super().__init__(oracle_mod, w, tri)
        self.f = band_centres(w.B, edges)
        self.dstats = dict(short_blocked=0, long_blocked=0, merged=0)

    def filter(self, S, L, own, margin, max_detour):
        """step 1 over all (triangle, edge) at once: (ok [T][3], the values the legs and the row use, each [T][3] or [T][3][3])"""
        S, L, m, md = np.asarray(S, np.float32), np.asarray(L, np.float32), F(margin), F(max_detour)
        v0, e1, e2 = self.v0, self.e1, self.e2
        with np.errstate(all="ignore"):
            n = cross(e1, e2)
            nn = dot(n, n)
            hS, hL = dot(S[None, :] - v0, n), dot(L[None, :] - v0, n)
            opposite = ((hS > 0) & (hL < 0)) | ((hS < 0) & (hL > 0))
            a = np.stack([v0, v0 + e1, v0 + e2], axis=1)
            w = np.stack([e1, e2 - e1, -e2], axis=1)
            n3 = np.broadcast_to(n[:, None, :], w.shape)
            ww = dot(w, w)
            o = cross(w, n3)
            oo = dot(o, o)
            rS, rL = S[None, None, :] - a, L[None, None, :] - a
            tS, tL = dot(rS, w) / ww, dot(rL, w) / ww
            cS, cL = cross(rS, w), cross(rL, w)
            dS, dL = np.sqrt(dot(cS, cS) / ww), np.sqrt(dot(cL, cL) / ww)
            total = dS + dL
            t = tS + ((tL - tS) * dS) / total
            E0 = fmaf_arrays(t[..., None], w, a)
            u, v = S[None, None, :] - E0, E0 - L[None, None, :]
            lS, lL = np.sqrt(dot(u, u)), np.sqrt(dot(v, v))
            length = lS + lL
            g = S - L
            distance = np.sqrt(dot(g, g))
            detour = length - distance
            s = hS / (hS - hL)
            X = fmaf_arrays(s[:, None], (L - S)[None, :], S[None, :])
            shadow = dot(X[:, None, :] - E0, o)
            ok = ((nn != 0) & opposite)[:, None] & (ww != 0) & (oo != 0) & (total != 0) & (t >= -m) & (t <= F(1.0) + m) & (lS != 0) & (lL != 0) & \
                (detour <= md) & (shadow <= 0)
        for x in (E0, length, detour, shadow, t, o):
            assert x.dtype == np.float32
        is_own = np.array([int(x) != NO_OBJECT and int(x) in own for x in self.w.obj], bool) if own else np.zeros(len(v0), bool)
        return ok & ~is_own[:, None], dict(E0=E0, u=u, v=v, lS=lS, lL=lL, length=length, detour=detour, o=o, oo=oo, n=n, nn=nn, hS=hS)

    def reached(self, o, d, length, own, step):
        return self.leg(o, d, length, own, -1, step)[0] == FREE

    def confirm(self, S32, L32, own, x, i, j, p):
        """step 2 for candidate (i, j): the short leg first, the verdicts are independent"""
        off = F(p["offset"])
        io = F(1.0) / np.sqrt(x["oo"][i, j])
        inn = F(1.0) / np.sqrt(x["nn"][i])
        sg = inn if x["hS"][i] > 0 else -inn
        nh = [F(x["n"][i, k] * sg) for k in range(3)]
        Eo = [fmaf(off, F(x["o"][i, j, k] * io), x["E0"][i, j, k]) for k in range(3)]
        ES = [fmaf(off, nh[k], Eo[k]) for k in range(3)]
        EL = [fmaf(-off, nh[k], Eo[k]) for k in range(3)]
        if not self.reached(ES, [-c for c in nh], F(F(2.0) * off), own, p["step"]):
            self.dstats["short_blocked"] += 1
            return False
        for start, end, back in ((S32, ES, None), (EL, L32, F(p["pullback"]))):
            e = np.array([F(end[k] - start[k]) for k in range(3)], np.float32)
            ln = F(np.sqrt(dot(e, e)))
            with np.errstate(all="ignore"):
                inv = F(1.0) / ln
                d = [F(e[k] * inv) for k in range(3)]
            if not self.reached(start, d, ln if back is None else F(ln - back), own, p["step"]):
                self.dstats["long_blocked"] += 1
                return False
        return True

    def row(self, S, L, src_obj=NO_OBJECT, lis_obj=NO_OBJECT, **params):
        """(row dict, the kept paths in the rule's order: all of them, not only max_paths)"""
        p = dict(DEFAULTS, **params)
        S32, L32 = [F(c) for c in S], [F(c) for c in L]
        own = {i for i in (src_obj, lis_obj) if i != NO_OBJECT}
        if len(self.v0) == 0:
            return dict(candidates=0, confirmed=0, found=0, returned=0, flags=0), []
        ok, x = self.filter(S32, L32, own, p["margin"], p["max_detour"])
        cand = np.argwhere(ok)
        if len(cand) > p["max_candidates"]:
            return dict(candidates=len(cand), confirmed=0, found=0, returned=0, flags=1), []
        conf = [(int(i), int(j)) for i, j in cand if self.confirm(S32, L32, own, x, int(i), int(j), p)]
        key = {c: (bits(x["length"][c]), 4 * c[0] + c[1]) for c in conf}
        mm = F(F(p["merge"]) * F(p["merge"]))
        kept = []
        for c in conf:
            q = [x["E0"][c] - x["E0"][d] for d in conf if key[d] < key[c]]
            if any(dot(qq, qq) < mm for qq in q):
                self.dstats["merged"] += 1
            else:
                kept.append(c)
        kept.sort(key=lambda c: key[c])
        paths = []
        for i, j in kept:
            length, detour, lS, lL = x["length"][i, j], x["detour"][i, j], x["lS"][i, j], x["lL"][i, j]
            gain = np.zeros(8, np.float32)
            for b in range(self.B):
                k = F(40.0 * self.f[b] / (float(F(p["sound_speed"])) * float(F(p["dist_divisor"]))))
                gain[b] = F(1.0) / np.sqrt(F(3.0) + k * detour)
            il = F(1.0) / lL
            paths.append(dict(length=length, delay=F(F(length / F(p["dist_divisor"])) / F(p["sound_speed"])), detour=detour,
                              cos_bend=dot(x["u"][i, j], x["v"][i, j]) / (lS * lL), apex=x["E0"][i, j], direction=x["v"][i, j] * il,
                              triangle=i, edge=j, material=int(self.w.mat[i]), gain=gain))
        return dict(candidates=len(cand), confirmed=len(conf), found=len(kept), returned=min(len(kept), p["max_paths"]), flags=0), paths

    def expect(self, pkg, positions, L, src_obj=None, lis_obj=NO_OBJECT, **params):
        """the call's two arrays as the library must write them"""
        mp = dict(DEFAULTS, **params)["max_paths"]
        rows = np.zeros(len(positions), dtype=pkg.Context.DIFFRACTION_ROW_DTYPE)
        paths = np.zeros((len(positions), mp), dtype=pkg.Context.DIFFRACTION_DTYPE)
        for i, S in enumerate(positions):
            r, ps = self.row(S, L, NO_OBJECT if src_obj is None else src_obj[i], lis_obj, **params)
            for k in rows.dtype.names:
                rows[i][k] = r[k]
            for j, y in enumerate(ps[:mp]):
                for k in paths.dtype.names:
                    paths[i, j][k] = y[k]
        return rows, paths


# ---- the scenes -----------------------------------------------------------------------------------------------------
SRC, LIS = [310.0, 230.0, 120.0], [720.0, 260.0, 110.0]          # either side of the partition
BSRC, BLIS = [300.0, 200.0, 120.0], [560.0, 450.0, 110.0]        # round the corner of the thick box
LIT = [520.0, 790.0, 110.0]                                      # sees SRC past the partition's side
SHEET = ((500.0, 0.0, 0.0), (0.0, 500.0, 0.0), (0.0, 0.0, 200.0))
BOX = ([450.0, 0.0, 0.0], [550.0, 400.0, 300.0])


def sheet_world(n=1, height=200.0, actor=2, material=OPAQUE):
    return shoebox_world([(quad_grid(SHEET[0], SHEET[1], (0.0, 0.0, height), n), material, actor)], n=n)


def box_world(n=1):
    return shoebox_world([(box(BOX[0], BOX[1], n), OPAQUE, 2)], n=n)


def unfold(S, L, a, w):
    """float64: (length, apex) of the shortest path S -> the line a + t w -> L"""
    S, L, a, w = (np.asarray(c, np.float64) for c in (S, L, a, w))
    ww = np.dot(w, w)
    tS, tL = np.dot(S - a, w) / ww, np.dot(L - a, w) / ww
    dS, dL = np.linalg.norm(np.cross(S - a, w)) / np.sqrt(ww), np.linalg.norm(np.cross(L - a, w)) / np.sqrt(ww)
    return float(np.hypot(dS + dL, (tL - tS) * np.sqrt(ww))), a + (tS + (tL - tS) * dS / (dS + dL)) * w


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.DiffractionParams) == 44 and C.sizeof(cap.DiffractionPath) == 84 and C.sizeof(cap.DiffractionRow) == 20
    assert pkg.Context.DIFFRACTION_DTYPE.itemsize == 84 and pkg.Context.DIFFRACTION_ROW_DTYPE.itemsize == 20
    P = cap.DiffractionPath
    assert (P.detour.offset, P.cos_bend.offset, P.apex.offset, P.direction.offset, P.triangle.offset, P.edge.offset, P.material.offset,
            P.gain.offset) == (8, 12, 16, 28, 40, 44, 48, 52)
    assert [pkg.Context.DIFFRACTION_DTYPE.fields[k][1] for k in ("detour", "cos_bend", "apex", "direction", "triangle", "edge", "material", "gain")] == \
        [8, 12, 16, 28, 40, 44, 48, 52]
    p = cap.default_diffraction_params()
    assert p.struct_size == 44
    assert (p.max_paths, p.max_candidates) == (4, 1024)
    assert p.margin == F(1e-3) and p.offset == F(0.1) and p.step == F(0.1) and p.pullback == F(0.1)
    assert p.max_detour == 1000.0 and p.merge == 1.0 and p.dist_divisor == 1000.0 and p.sound_speed == 343.0
    assert (cap.MAX_DIFFRACTIONS, cap.MAX_DIFFRACTION_CANDIDATES, cap.MAX_DIFFRACTION_BATCH, cap.DIFFRACTION_OVERFLOW) == (16, 2048, 256, 1)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frequensee.h")).read()
    for name, value in (("FS_MAX_DIFFRACTIONS", "16"), ("FS_MAX_DIFFRACTION_CANDIDATES", "2048"), ("FS_MAX_DIFFRACTION_BATCH", "256"),
                        ("FS_DIFFRACTION_OVERFLOW", "1u")):
        assert f"#define {name}" in header and header.split(f"#define {name}")[1].split()[0] == value
    assert cap.load().fs_abi_version() == 5, "the change only adds"
    assert band_centres(8) == pytest.approx([125.0 * 2 ** b for b in range(8)], rel=1e-12)


def test_exported_in_one_tier(pkg):
    contract.exported_in_one_tier(pkg, ("fs_diffraction_params_default", "fs_update_diffraction_paths"))


def test_null_context_and_no_device(pkg):
    contract.null_context_and_no_device(pkg, QUERY)


# fp32 against float64: the chain to a length is S - a (1), the two dots and ww (5 each), two divides, two crosses (3 per component),
# their squares (5 each), two divides and square roots, the sum, t (4), the fmaf, u and v (1 each), their squares (5 each), two square
# roots and the sum — about forty roundings of 6e-8 each where test_restatement_against_image_sources has twenty: twice its 1e-5, the
# same order of margin.  The apex is held to the same figure on the room's size, times ten as the reflection point is there.
LENGTH_RTOL = 2e-5
SIZE = 1000.0


def check_path(p, ref_length, ref_apex, S, L):
    assert abs(float(p["length"]) - ref_length) <= LENGTH_RTOL * ref_length, (p["length"], ref_length)
    assert np.allclose(p["apex"], ref_apex, rtol=0, atol=LENGTH_RTOL * SIZE * 10), (p["apex"], ref_apex)
    straight = float(np.linalg.norm(np.asarray(S, np.float64) - np.asarray(L, np.float64)))
    assert p["detour"] > 0 and abs(float(p["detour"]) - (ref_length - straight)) <= 2 * LENGTH_RTOL * ref_length
    d = (ref_apex - np.asarray(L, np.float64)) / np.linalg.norm(ref_apex - np.asarray(L, np.float64))
    assert np.allclose(p["direction"], d, rtol=0, atol=1e-4)
    a, b = ref_apex - np.asarray(S, np.float64), np.asarray(L, np.float64) - ref_apex
    assert abs(float(p["cos_bend"]) - float(np.dot(a, b) / np.linalg.norm(a) / np.linalg.norm(b))) <= 1e-5
    g = p["gain"]
    assert np.all(g[:4] > 0) and np.all(np.diff(g[:4]) < 0) and g[0] < 1.0 / np.sqrt(3.0) and np.all(g[4:] == 0)
    k = [40.0 * f / (343.0 * 1000.0) for f in (125.0, 250.0, 500.0, 1000.0)]
    assert np.allclose(g[:4], [1.0 / np.sqrt(3.0 + kb * (ref_length - straight)) for kb in k], rtol=1e-4)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_restatement_single_sheet_partition(pkg, oracle_mod, n):
    """over the top edge and round the side edge of a single sheet; the interior edges, the edge on the floor and the edge on the wall
    are candidates the short leg or a long one rejects"""
    top = unfold(SRC, LIS, (500.0, 0.0, 200.0), (0.0, 500.0, 0.0))
    side = unfold(SRC, LIS, (500.0, 500.0, 0.0), (0.0, 0.0, 200.0))
    assert abs(top[0] - 444.8653) < 5e-4 and np.allclose(top[1], (500.0, 243.934, 200.0), atol=5e-3)
    assert abs(side[0] - 655.8041) < 5e-4 and np.allclose(side[1], (500.0, 500.0, 114.965), atol=5e-3)
    for (_, apex), axis, extent in ((top, 1, 500.0), (side, 2, 200.0)):   # (on the input) no apex near the end of a sub-edge
        t = apex[axis] / (extent / n)
        assert min(t - np.floor(t), np.ceil(t) - t) > 0.02
    w = sheet_world(n)
    y = Diffraction(oracle_mod, w)
    r, paths = y.row(SRC, LIS)
    assert r == dict(candidates={1: 5, 2: 10, 4: 16}[n], confirmed=2, found=2, returned=2, flags=0), r
    assert y.dstats["short_blocked"] > 0
    first = 12 * n * n   # the partition's triangles follow the room's
    assert all(p["triangle"] >= first for p in paths)
    check_path(paths[0], top[0], top[1], SRC, LIS)
    check_path(paths[1], side[0], side[1], SRC, LIS)
    assert paths[0]["length"] < paths[1]["length"] and paths[0]["gain"][3] > paths[1]["gain"][3]
    # the direct line is blocked
    e = np.asarray(LIS, np.float32) - np.asarray(SRC, np.float32)
    ln = F(np.sqrt(dot(e, e)))
    assert not y.reached([F(c) for c in SRC], [F(c / ln) for c in e], ln, set(), 0.1)
    # a lit listener has no path; a listener on the source's side not even a candidate
    assert y.reached([F(c) for c in SRC], [F(c) for c in (np.asarray(LIT) - np.asarray(SRC)) / np.linalg.norm(np.asarray(LIT) - np.asarray(SRC))],
                     F(np.linalg.norm(np.asarray(LIT) - np.asarray(SRC))), set(), 0.1)
    assert y.row(SRC, LIT)[0]["found"] == 0
    assert y.row(SRC, [400.0, 600.0, 50.0])[0]["candidates"] == 0


@pytest.mark.parametrize("n", [1, 2, 4])
def test_restatement_thick_box_corner(pkg, oracle_mod, n):
    """a convex corner is confirmed once from each of its faces and merged into one path"""
    corner = unfold(BSRC, BLIS, (450.0, 400.0, 0.0), (0.0, 0.0, 300.0))
    assert abs(corner[0] - 370.965) < 5e-3 and np.allclose(corner[1], (450.0, 400.0, 113.26), atol=5e-3)
    t = corner[1][2] / (300.0 / n)
    assert min(t - np.floor(t), np.ceil(t) - t) > 0.02
    y = Diffraction(oracle_mod, box_world(n))
    r, paths = y.row(BSRC, BLIS)
    assert (r["confirmed"], r["found"], r["returned"], r["flags"]) == (2, 1, 1, 0), r
    assert y.dstats["merged"] == 1
    check_path(paths[0], corner[0], corner[1], BSRC, BLIS)
    r, paths = y.row(BSRC, BLIS, merge=0.0)
    assert (r["confirmed"], r["found"]) == (2, 2) and np.allclose(paths[0]["apex"], paths[1]["apex"], atol=1e-3)
    assert {p["triangle"] // (2 * n * n) - 6 for p in paths} == {0, 3}, "one entry from the x lo face, one from the y hi face"


# ---- GPU ---------------------------------------------------------------------------------------------------------------
check = contract.checker("diffraction")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4], ids=["one_workgroup", "several_workgroups"])
def test_partition_and_corner(pkg, oracle_mod, n):
    w = sheet_world(n)
    assert len(w.tri) < 256, "the partition's scenes: one scan workgroup, partly full"
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Diffraction(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, f"partition n={n}")
    assert tuple(rows[0]) == ({1: 5, 4: 16}[n], 2, 2, 2, 0)
    assert np.all(paths[0][2:].view(np.uint8) == 0)
    ctx.set_listener(LIT)
    rows, _ = check(pkg, ctx, Diffraction(oracle_mod, w), place(ctx, [SRC]), [SRC], LIT, "lit")
    assert rows[0]["found"] == 0
    ctx.close()
    w = box_world(n)
    assert (len(w.tri) > 256) == (n == 4), "the box's scenes: one scan workgroup, and several"
    ctx = w.context(pkg)
    ctx.set_listener(BLIS)
    h = place(ctx, [BSRC])
    rows, paths = check(pkg, ctx, Diffraction(oracle_mod, w), h, [BSRC], BLIS, f"corner n={n}")
    assert tuple(rows[0])[1:] == (2, 1, 1, 0)
    rows, paths = check(pkg, ctx, Diffraction(oracle_mod, w), h, [BSRC], BLIS, f"corner n={n}, no merge", merge=0.0)
    assert tuple(rows[0])[1:] == (2, 2, 2, 0)
    ctx.close()


@pytest.mark.gpu
def test_wall_to_the_ceiling_and_own_actor(pkg, oracle_mod):
    w = sheet_world(2, height=300.0)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Diffraction(oracle_mod, w), place(ctx, [SRC]), [SRC], LIS, "to the ceiling")
    assert tuple(rows[0])[1:] == (1, 1, 1, 0) and abs(float(paths[0][0]["apex"][1]) - 500.0) < 1e-3, "only round the side"
    ctx.close()
    # the partition as the source's own actor: passed, no path; under a foreign id: paths
    w = sheet_world(2, actor=8)
    y = Diffraction(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, _ = check(pkg, ctx, y, h, [SRC], LIS, "foreign id")
    assert tuple(rows[0])[1:] == (2, 2, 2, 0)
    ctx.set_source_object(h[0], 8)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "own actor", src_obj=[8])
    assert tuple(rows[0]) == (0, 0, 0, 0, 0) and np.all(paths.view(np.uint8) == 0)
    ctx.set_source_object(h[0], NO_OBJECT)
    ctx.set_listener_object(8)
    rows, _ = check(pkg, ctx, y, h, [SRC], LIS, "the listener's actor", lis_obj=8)
    assert tuple(rows[0]) == (0, 0, 0, 0, 0)
    ctx.close()


@pytest.mark.gpu
def test_caps(pkg, oracle_mod):
    w = sheet_world(2)
    y = Diffraction(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    full = ctx.diffraction_paths(h)
    assert tuple(full[0][0]) == (10, 2, 2, 2, 0)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "the shortest", max_paths=1)
    assert tuple(rows[0]) == (10, 2, 2, 1, 0) and paths.shape == (1, 1) and paths[0].tobytes() == full[1][0][:1].tobytes()
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "exactly the cap", max_candidates=10, max_paths=16)
    assert tuple(rows[0]) == (10, 2, 2, 2, 0) and paths.shape == (1, 16)
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "one below", max_candidates=9)
    assert tuple(rows[0]) == (10, 0, 0, 0, pkg._capi.DIFFRACTION_OVERFLOW) and np.all(paths.view(np.uint8) == 0)
    assert full[1][0]["detour"][0] < 100.0 < full[1][0]["detour"][1]
    rows, paths = check(pkg, ctx, y, h, [SRC], LIS, "max_detour", max_detour=100.0)
    assert tuple(rows[0])[1:] == (1, 1, 1, 0) and rows[0]["candidates"] < 10 and paths[0][0].tobytes() == full[1][0][0].tobytes()
    ctx.close()


@pytest.mark.gpu
def test_materials_and_degenerate_triangles(pkg, oracle_mod):
    room = box(LO, HI)
    sheet = np.asarray(quad_grid(SHEET[0], SHEET[1], SHEET[2], 2), np.float32)
    degenerate = np.array([[[500.0, 100.0, 250.0], [500.0, 100.0, 250.0], [500.0, 300.0, 260.0]],      # two corners equal
                           [[500.0, 0.0, 210.0], [500.0, 200.0, 230.0], [500.0, 400.0, 250.0]],        # three on a line
                           [[500.0, 300.0, 220.0], [500.0, 300.0, 220.0], [500.0, 300.0, 220.0]]], np.float32)   # a point
    # the sheet's triangles: no material, an id beyond the table, material 0; three bands
    w = World([(room, 0, 1), (sheet[0:3], NO_MATERIAL, 2), (sheet[3:6], 9, 2), (sheet[6:8], 0, 2), (degenerate, 0, 2)],
              [a[:3] for a in ALPHA], [t[:3] for t in TAU], 3, [x[:3] for x in SCAT])
    y = Diffraction(oracle_mod, w)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, y, place(ctx, [SRC]), [SRC], LIS, "materials")
    assert tuple(rows[0])[1:] == (2, 2, 2, 0)
    assert {int(m) for m in paths[0]["material"][:2]} <= {NO_MATERIAL, 9, 0} and len({int(m) for m in paths[0]["material"][:2]}) == 2
    for p in paths[0][:2]:
        assert p["material"] == w.mat[p["triangle"]] and np.all(p["gain"][:3] > 0) and np.all(p["gain"][3:] == 0)
    for k in ("length", "delay", "detour", "cos_bend", "apex", "direction", "gain"):
        assert np.all(np.isfinite(paths[k]))
    ctx.close()


_rooms = {}


def rooms_case(pkg, oracle_mod):
    """starter_room, 64 seeded sources, the scene's listener, and the restatement's arrays — computed once"""
    if not _rooms:
        sc = pkg.scenes.starter_room(4)
        tr, sca = pkg.scenes.material_lobes(sc)
        w = World([], sc.absorption, tr, 4, sca)
        w.tri, w.mat, w.obj = sc.triangles.astype(np.float32), sc.material_ids.astype(np.uint16), sc.object_ids.astype(np.uint32)
        rng = np.random.default_rng(0xD1FF)
        lo, hi = w.tri.reshape(-1, 3).min(axis=0), w.tri.reshape(-1, 3).max(axis=0)
        pos = rng.uniform(lo, hi, (64, 3)).astype(np.float32)
        _rooms.update(w=w, pos=pos, lis=sc.listener, want=Diffraction(oracle_mod, w).expect(pkg, pos, sc.listener, max_detour=3000.0))
    return _rooms


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["sah", "device_morton"])
def test_rooms(pkg, oracle_mod, fast):
    rc = rooms_case(pkg, oracle_mod)
    ctx = rc["w"].context(pkg, fast=fast)
    ctx.set_listener(rc["lis"])
    h = place(ctx, rc["pos"])
    rows, paths = got = ctx.diffraction_paths(h, max_detour=3000.0)
    assert_equal(got, rc["want"], f"rooms fast={fast}")
    # the case is not trivial: the wave strides more than once, and every stage removes something somewhere
    assert np.any(rows["candidates"] > 64) and len(set(rows["found"])) > 2
    assert np.any(rows["confirmed"] < rows["candidates"]) and np.any(rows["found"] < rows["confirmed"])
    contract.batch_agrees(ctx.diffraction_paths, h, got, singles=not fast, max_detour=3000.0)
    ctx.close()


@pytest.mark.gpu
def test_mover(pkg, oracle_mod):
    """a wall to the ceiling with a door in the same plane that shuts the gap beside it: no path; the door slid out of the room: the
    path round the wall's side; the door back: none"""
    wall = quad_grid(SHEET[0], SHEET[1], (0.0, 0.0, 300.0), 1)
    door = quad_grid((500.0, 500.0, 0.0), (0.0, 300.0, 0.0), (0.0, 0.0, 300.0), 1)
    w = shoebox_world([(wall, OPAQUE, 2), (door, OPAQUE, 5)])
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    rows, _ = check(pkg, ctx, Diffraction(oracle_mod, w), h, [SRC], LIS, "door shut")
    assert rows[0]["candidates"] > 0 and rows[0]["found"] == 0
    aside = np.array([[1, 0, 0, 0], [0, 1, 0, 400], [0, 0, 1, 0]], np.float32)
    ctx.set_object_transforms([5], aside[None])
    rows, paths = check(pkg, ctx, Diffraction(oracle_mod, w, contract.transformed(w, 5, aside)), h, [SRC], LIS, "door aside, no explicit refit")   # the call refits first
    assert rows[0]["found"] == 1 and abs(float(paths[0][0]["apex"][1]) - 500.0) < 1e-3 and paths[0][0]["triangle"] in (12, 13)
    ctx.set_object_transforms([5], np.eye(3, 4, dtype=np.float32)[None])
    rows, _ = check(pkg, ctx, Diffraction(oracle_mod, w), h, [SRC], LIS, "door back")
    assert rows[0]["found"] == 0
    ctx.close()


def _defaults_found(t, oracle_mod, want):
    assert tuple(want[0][0]) == (5, 2, 2, 2, 0)


def _legal_found(rows):
    assert tuple(rows[0]) == (5, 0, 0, 0, 1)


inf, nan = float("inf"), float("nan")
QUERY = contract.Query(
    kind="diffraction", dtypes=("DIFFRACTION_ROW_DTYPE", "DIFFRACTION_DTYPE"), world=lambda: sheet_world(1), src=SRC, lis=LIS, wrong_struct_size=40,
    null_paths=4, refused_without_device=(dict(max_detour=0.0),),
    refused=(dict(max_paths=0), dict(max_paths=17), dict(max_candidates=0), dict(max_candidates=2049), dict(margin=-1e-3), dict(margin=nan),
             dict(margin=inf), dict(max_detour=0.0), dict(max_detour=-1.0), dict(max_detour=nan), dict(max_detour=inf), dict(offset=-0.1),
             dict(offset=nan), dict(offset=inf), dict(merge=-1.0), dict(merge=nan), dict(merge=inf), dict(step=-0.1), dict(step=nan),
             dict(step=inf), dict(pullback=-1.0), dict(pullback=nan), dict(pullback=inf), dict(dist_divisor=0.0), dict(dist_divisor=-1.0),
             dict(dist_divisor=nan), dict(dist_divisor=inf), dict(sound_speed=0.0), dict(sound_speed=-1.0), dict(sound_speed=nan),
             dict(sound_speed=inf)),
    defaults_found=_defaults_found,
    legal=(dict(max_paths=16, max_candidates=2048, margin=0.0, offset=0.0, merge=0.0, step=0.0, pullback=0.0), dict(max_paths=16, max_candidates=1)),
    legal_found=_legal_found, yardstick=Diffraction,
    empty_world=lambda: World([], ALPHA, TAU, 4, SCAT), fewer=dict(max_paths=16, max_candidates=2048))


@pytest.mark.gpu
def test_errors_and_untouched_state(pkg, oracle_mod):
    contract.errors_and_untouched_state(pkg, oracle_mod, QUERY)


@pytest.mark.gpu
def test_band_edges_in_force(pkg, oracle_mod):
    """k_b follows fs_set_band_edges; a single band has f_0 = 1000 Hz"""
    w = sheet_world(1)
    ctx = w.context(pkg)
    ctx.set_listener(LIS)
    h = place(ctx, [SRC])
    check(pkg, ctx, Diffraction(oracle_mod, w), h, [SRC], LIS, "default edges")
    edges = [300.0, 1200.0, 5000.0]
    ctx.set_band_edges(edges)
    rows, paths = check(pkg, ctx, Diffraction(oracle_mod, w, edges=edges), h, [SRC], LIS, "edges given")
    ctx.set_band_edges(None)
    check(pkg, ctx, Diffraction(oracle_mod, w), h, [SRC], LIS, "default edges again")
    ctx.close()
    one = World([(box(LO, HI), 0, 1), (quad_grid(*SHEET, 1), 0, 2)], [[0.5]], [[0.0]], 1, [[0.5]])
    ctx = one.context(pkg)
    ctx.set_listener(LIS)
    rows, paths = check(pkg, ctx, Diffraction(oracle_mod, one), place(ctx, [SRC]), [SRC], LIS, "one band")
    assert rows[0]["found"] == 2 and np.all(paths[0]["gain"][:2, 0] > 0) and np.all(paths[0]["gain"][:, 1:] == 0)
    ctx.close()


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    contract.steady_state_allocates_nothing(pkg, QUERY)


def interleaved_positions():
    """33 seeded positions, the even ones on SRC's side of the partition and the odd ones on the listener's"""
    pos = np.random.default_rng(0x1A7E).uniform([50.0, 50.0, 40.0], [450.0, 750.0, 260.0], (33, 3)).astype(np.float32)
    pos[1::2, 0] += np.float32(500.0)
    return pos


@pytest.mark.gpu
def test_queries_interleaved_on_one_context(pkg):
    """the three queries share their chain, scan and staging code but no buffer: on one context, in an order in which every staging is
    used (count 5: a confirm workgroup with three idle waves; count 1), then grown past its first capacity of 32 (count 33), then used
    again with fewer rows, each call returns the bytes it returns as the first call of a fresh context"""
    w = sheet_world(4)
    assert len(w.tri) == 224
    pos = interleaved_positions()
    assert np.any(pos[:, 0] < 500.0) and np.any(pos[:, 0] > 500.0)

    def fresh():
        ctx = w.context(pkg)
        ctx.set_listener(LIS)
        return ctx, place(ctx, pos)

    calls = [("diffraction", 5), ("direct", 33), ("reflection", 1), ("diffraction", 33), ("reflection", 33), ("direct", 5), ("reflection", 5),
             ("diffraction", 1)]
    got = contract.queries_interleaved_on_one_context(fresh, calls, {})
    # the comparison is not of zeros
    direct, diffraction, reflection = got[1][0], got[3], got[4]
    assert np.any(direct["visibility"] < 1.0) and np.any(direct["visibility"] == 1.0)
    assert np.any(reflection[0]["returned"] > 0) and np.any(diffraction[0]["returned"] > 0)


@pytest.mark.gpu
def test_component_layer(pkg, oracle_mod):
    """a source walks behind the partition: UpdateDiffractionPaths is Context.diffraction_paths over the active sources, Voices()
    appends a diffraction voice whose key no reflection has, and the callback it appears in reports it as started"""
    from test_direct_render import noise
    w = sheet_world(1)
    frame, taps = 64, 15
    sub = pkg.AudioRayTracingSubsystem(num_bands=4)
    sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
    sub.SetMaterials(w.absorption, w.transmission, w.scattering)
    # a step across the shadow boundary of the partition's side edge (the listener's line past (500, 500) reaches x = 310 at y = 707):
    # the listener sees the first position; at the second every reflection is one the first had, so the only new voice is the bent one
    lit, hidden = [310.0, 720.0, 120.0], [310.0, 690.0, 120.0]
    comp = pkg.FrequenSeeAudioComponent(lit)
    comp.OnRegister(sub)
    sub.SetListenerLocation(LIS)
    plug = pkg.FrequenSeeAudioReflectionPlugin(sub)
    plug.Initialize(frame, taps, 32, 0.05)
    plug.OnInitSource(comp)
    rng = np.random.default_rng(5)
    y = Diffraction(oracle_mod, w)
    seen = []
    for cb, pos in enumerate((lit, lit, hidden, hidden)):
        comp.SetComponentLocation(pos)
        rows, paths = sub.UpdateReflectionPaths(max_paths=8)
        drows, dpaths = got = sub.UpdateDiffractionPaths(max_paths=1)
        assert_equal(got, y.expect(pkg, [pos], LIS, max_paths=1), f"component layer, callback {cb}")
        voices = plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0], diffraction=(drows[0], dpaths[0]))
        nr, nd = int(rows[0]["returned"]), int(drows[0]["returned"])
        assert voices.shape == (nr + nd,) and nd == (1 if cb >= 2 else 0)
        assert np.array_equal(voices[:nr], plug.Voices(rows[0], paths[0], right=[0.0, 1.0, 0.0])), "the reflections' voices changed"
        out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, right=[0.0, 1.0, 0.0], diffraction=(drows, dpaths))
        assert int(counts[0]["dropped"]) == 0
        if nd:
            v = voices[nr]
            assert int(v["key"]) == 0x80000000 | (int(dpaths[0][0]["triangle"]) * 4 + int(dpaths[0][0]["edge"]))
            assert int(v["key"]) not in {int(k) for k in voices["key"][:nr]} and np.all(voices["key"][:nr] < 0x80000000)
            assert np.array_equal(v["band_gain"], dpaths[0][0]["gain"])
            assert float(v["delay"]) == pytest.approx(float(dpaths[0][0]["delay"]) - ((taps - 1) // 2) / sub.ctx.cfg.sample_rate, abs=1e-7)
        seen.append((set(int(k) for k in voices["key"]), int(counts[0]["started"])))
    # callback 2 is the one the diffraction voice appears in: it is the only new key, and started == 1
    new = seen[2][0] - seen[1][0]
    assert len(new) == 1 and all(k & 0x80000000 for k in new) and seen[2][1] == 1
    assert seen[3][1] == 0 and seen[3][0] == seen[2][0], "a steady source starts nothing"
    plug.OnReleaseSource(comp)
    sub.Deinitialize()
