"""fs_pathing_*: the probe graph that carries a source's sound round several corners, and fs_update_pathing_paths.

The yardstick is a Python restatement of include/frequensee.h's "pathing" rule on numpy float32 (every operation rounded on its
own): the pair lengths as float32 array arithmetic, every chain as the max_surfaces = 0 leg of tests/test_reflection_paths.py round
oracle.Scene.trace_closest(brute=True), the relaxation as Jacobi rounds, k_b from the test's own band centres.  Every word of the
graph and every field of every row must EQUAL it, floats by bit pattern.  The restatement itself is checked without a GPU: its
distances against a float64 Dijkstra under a bound derived from the rule's roundings, and Jacobi against in-place relaxation.
"""
import ctypes as C
import functools
import heapq
import os

import numpy as np
import pytest

pytest.register_assert_rewrite("path_query_contract")
import path_query_contract as contract  # noqa: E402
from test_diffraction_paths import band_centres
from test_reflection_paths import (ALPHA, FREE, NO_OBJECT, OPAQUE, SCAT, TAU, WALLS, F, Restatement, World, bits, box, dot,
                                   place, quad_grid)

DEFAULTS = dict(validate=1, max_attach=1000.0, max_length=10000.0, step=0.1, pullback=0.1, dist_divisor=1000.0, sound_speed=343.0)
BAKE_DEFAULTS = dict(max_edge=1000.0, step=0.1)
FOUND, DIRECT, STALE = 1, 2, 4
NO_PROBE = 0xFFFFFFFF
LISTENER = -1
NODES = 16
KEY = 0x80000003
INF = F(np.inf)
U = 2.0 ** -24


def norm32(e):
    """sqrtf(e.e) on float32 arrays [..., 3]"""
    return np.sqrt(dot(e, e))


class Pathing:
    """the rule of the header for one world and one probe set"""

    def __init__(self, oracle_mod, w, probes, tri=None):
        self.y = Restatement(oracle_mod, w, tri)
        self.P = np.ascontiguousarray(probes, np.float32).reshape(-1, 3)
        self.N = len(self.P)
        self.k = None
        e = self.P[None, :, :] - self.P[:, None, :]   # e[i, j] = p_j - p_i
        self.e, self.w = e, norm32(e)                 # w is symmetric to the bit: only squares enter
        assert np.array_equal(self.w.view(np.uint32), self.w.T.view(np.uint32))
        self.chains = 0

    def reached(self, o, e, a, own, step):
        """chain(o, e (1.0f / a), a') with max_surfaces = 0; a' = a unless given as a pair (a, len)"""
        a, length = a if isinstance(a, tuple) else (a, a)
        self.chains += 1
        if self.y.sc is None:
            return True
        inv = F(1.0) / F(a)
        d = [F(F(e[i]) * inv) for i in range(3)]
        return self.y.leg([F(x) for x in o], d, F(length), own, -1, step)[0] == FREE

    def bake(self, **params):
        p = dict(BAKE_DEFAULTS, **params)
        n = self.N
        cand = np.triu(np.ones((n, n), bool), 1) & (self.w >= F(1.0)) & (self.w <= F(p["max_edge"]))
        adj = np.zeros((n, n), bool)
        for i, j in np.argwhere(cand):
            if self.reached(self.P[i], self.e[i, j], self.w[i, j], set(), p["step"]):
                adj[i, j] = adj[j, i] = True
        self.adj = adj
        self.nbr = [np.nonzero(adj[i])[0] for i in range(n)]
        return self

    def graph(self):
        out = np.zeros((self.N, (self.N + 31) // 32), np.uint32)
        for i, j in np.argwhere(self.adj):
            out[i, j >> 5] |= np.uint32(1 << (j & 31))
        return out

    def edges(self):
        return int(self.adj.sum()) // 2

    def attach(self, L, lo, max_attach, step):
        L = np.asarray(L, np.float32)
        e = self.P - L[None, :]
        a = norm32(e)
        dL = np.full(self.N, INF, np.float32)
        own = {lo} if lo != NO_OBJECT else set()
        for k in range(self.N):
            if a[k] > F(max_attach):
                continue
            if a[k] == 0:
                dL[k] = F(0.0)
            elif self.reached(L, e[k], a[k], own, step):
                dL[k] = a[k]
        return dL

    def relax(self, dL, max_length, order="jacobi"):
        """(d, pred, rounds): rounds = the rounds that changed something"""
        d, ml, rounds = dL.copy(), F(max_length), 0
        with np.errstate(invalid="ignore"):
            for _ in range(self.N):
                if order == "jacobi":
                    c = d[:, None] + self.w                       # c[j, i] = d[j] + w_ji
                    c = np.where(self.adj & (c <= ml), c, INF)
                    new = np.minimum(d, c.min(axis=0)) if self.N else d
                else:
                    new = d.copy()
                    for i in (range(self.N) if order == "inplace" else reversed(range(self.N))):
                        for j in self.nbr[i]:
                            c = F(new[j] + self.w[j, i])
                            if c <= ml and c < new[i]:
                                new[i] = c
                assert new.dtype == np.float32
                if np.array_equal(new.view(np.uint32), d.view(np.uint32)):
                    break
                d, rounds = new, rounds + 1
            else:
                c = d[:, None] + self.w
                assert np.array_equal(np.minimum(d, np.where(self.adj & (c <= ml), c, INF).min(axis=0)).view(np.uint32), d.view(np.uint32)), \
                    "no fixed point after N rounds"
        pred = np.full(self.N, LISTENER, np.int64)
        for i in range(self.N):
            if bits(d[i]) != bits(dL[i]):
                pred[i] = next(j for j in self.nbr[i] if F(d[j] + self.w[j, i]) <= ml and bits(F(d[j] + self.w[j, i])) == bits(d[i]))
        return d, pred, rounds

    def listener(self, L, lo=NO_OBJECT, **params):
        p = dict(DEFAULTS, **params)
        self.L, self.lo = np.asarray(L, np.float32), lo
        self.dL = self.attach(L, lo, p["max_attach"], p["step"])
        self.d, self.pred, self.rounds = self.relax(self.dL, p["max_length"])
        return self

    def unit(self, origin, points):
        for q in points:
            v = np.asarray(q, np.float32) - origin
            n = norm32(v)
            if n != 0:
                return v * (F(1.0) / n)
        return np.zeros(3, np.float32)

    def row(self, S, so=NO_OBJECT, **params):
        """the source's row as a dict, and the totals of every qualifying probe"""
        p = dict(DEFAULTS, **params)
        S, L = np.asarray(S, np.float32), self.L
        own = {i for i in (so, self.lo) if i != NO_OBJECT}
        g = S - L
        distance = norm32(g)
        direct = distance == 0 or self.reached(S, -g, (distance, F(distance - F(p["pullback"]))), own, p["step"])
        e = self.P - S[None, :]
        a = norm32(e)
        totals = {}
        for k in range(self.N):
            if not (self.d[k] < INF) or not (a[k] <= F(p["max_attach"])):
                continue
            if a[k] == 0 or self.reached(S, e[k], a[k], own, p["step"]):
                total = F(self.d[k] + a[k])
                if total <= F(p["max_length"]):
                    totals[k] = total
        r = dict(length=F(0), delay=F(0), detour=F(0), distance=distance, direction=np.zeros(3, np.float32), departure=np.zeros(3, np.float32), hops=0,
                 flags=DIRECT if direct else 0, first_probe=0, last_probe=0, probes=np.zeros(NODES, np.uint32), gain=np.zeros(8, np.float32))
        if not totals:
            return r, totals
        k = min(totals, key=lambda q: (bits(totals[q]), q))
        back = [k]
        while self.pred[back[-1]] != LISTENER:
            back.append(int(self.pred[back[-1]]))
        seq = back[::-1]   # from the listener's end
        total = totals[k]
        stale = False
        if p["validate"]:
            for a_, b_ in zip(seq, seq[1:]):
                i, j = min(a_, b_), max(a_, b_)
                stale = stale or not self.reached(self.P[i], self.e[i, j], self.w[i, j], set(), p["step"])
        detour = F(total - distance)
        f = band_centres(self.y.B)
        for b in range(self.y.B):
            kb = F(40.0 * f[b] / (float(F(p["sound_speed"])) * float(F(p["dist_divisor"]))))
            r["gain"][b] = F(1.0) / np.sqrt(F(F(3.0) + kb * detour))
        r.update(length=total, delay=F(F(total / F(p["dist_divisor"])) / F(p["sound_speed"])), detour=detour, hops=len(seq),
                 flags=FOUND | (DIRECT if direct else 0) | (STALE if stale else 0), first_probe=seq[0], last_probe=seq[-1],
                 probes=np.array((seq + [NO_PROBE] * NODES)[:NODES], np.uint32),
                 direction=self.unit(L, [self.P[q] for q in seq] + [S]), departure=self.unit(S, [self.P[q] for q in back] + [L]))
        return r, totals

    def expect(self, pkg, positions, src_obj=None, **params):
        out = np.zeros(len(positions), dtype=pkg.Context.PATHING_DTYPE)
        for i, S in enumerate(positions):
            r, _ = self.row(S, NO_OBJECT if src_obj is None else src_obj[i], **params)
            for k in out.dtype.names:
                out[i][k] = r[k]
        return out


def assert_rows(got, want, where=""):
    assert got.shape == want.shape and got.dtype == want.dtype, where
    for i in range(len(want)):
        for k in want.dtype.names:
            g, x = np.atleast_1d(got[i][k]), np.atleast_1d(want[i][k])
            assert g.tobytes() == x.tobytes(), f"{where} row {i}: {k}: got {g!r}, restatement {x!r}"
    assert got.tobytes() == want.tobytes(), where


# ---- the scenes -----------------------------------------------------------------------------------------------------
LO, HI = [0.0, 0.0, 0.0], [900.0, 400.0, 300.0]
Z = 140.0   # (off the walls' tessellation lines at z = 150)
LIS, SRC = [100.0, 310.0, Z], [800.0, 110.0, Z]
DOOR_ACTOR = 5
SHUT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -2000]], np.float32)   # the door's rest pose is 2000 cm above its frame
REST = np.eye(3, 4, dtype=np.float32)


def three_rooms(door=False):
    """a box split at x = 300 by a partition with a door frame y 40 .. 120, floor to ceiling, and at x = 600 by a wall that hangs
    from the ceiling down to z = 100: the two openings' edges are a jamb (along z) and a lintel (along y), so no pair of parallel
    edges and no single edge joins the outer rooms.  door: a leaf for the frame, actor 5, resting 2000 cm above it"""
    parts = [(box(LO, HI, 2), WALLS, 1),
             (quad_grid((300.0, 0.0, 0.0), (0.0, 40.0, 0.0), (0.0, 0.0, 300.0), 2), OPAQUE, 2),
             (quad_grid((300.0, 120.0, 0.0), (0.0, 280.0, 0.0), (0.0, 0.0, 300.0), 2), OPAQUE, 2),
             (quad_grid((600.0, 0.0, 100.0), (0.0, 400.0, 0.0), (0.0, 0.0, 200.0), 2), OPAQUE, 2)]
    if door:
        parts.append((quad_grid((300.0, 40.0, 2000.0), (0.0, 80.0, 0.0), (0.0, 0.0, 300.0), 1), OPAQUE, DOOR_ACTOR))
    return World(parts, ALPHA, TAU, 4, SCAT)


def room_probes():
    """three by three per room at z = 140, one either side of the door frame, one under the hanging wall: 30"""
    grid = [[x, y, Z] for x in (60.0, 150.0, 240.0, 370.0, 460.0, 550.0, 660.0, 750.0, 840.0) for y in (70.0, 210.0, 330.0)]
    return np.array(grid + [[280.0, 80.0, Z], [320.0, 80.0, Z], [600.0, 210.0, 50.0]], np.float32)


ROOMS_BAKE = dict(max_edge=250.0)


@functools.lru_cache(maxsize=None)
def rooms_case(oracle_mod):
    """the three rooms, baked, with the listener in the first room: shared, never changed"""
    w = three_rooms()
    return w, Pathing(oracle_mod, w, room_probes()).bake(**ROOMS_BAKE).listener(LIS)


def rooms_sources():
    """SRC, then 63 seeded positions all over the three rooms"""
    pos = np.random.default_rng(0x9A7).uniform([20.0, 20.0, 20.0], [880.0, 380.0, 280.0], (64, 3)).astype(np.float32)
    pos[0] = SRC
    return pos


def graph_of(ctx):
    return ctx.pathing_graph()


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.PathingBakeParams) == 12 and C.sizeof(cap.PathingParams) == 32 and C.sizeof(cap.PathingPath) == 152
    assert pkg.Context.PATHING_DTYPE.itemsize == 152
    assert pkg.Context.PATHING_DTYPE.names == tuple(k for k, _ in cap.PathingPath._fields_)
    for name in pkg.Context.PATHING_DTYPE.names:
        assert pkg.Context.PATHING_DTYPE.fields[name][1] == getattr(cap.PathingPath, name).offset
    b = cap.default_pathing_bake_params()
    assert (b.struct_size, b.max_edge, b.step) == (12, 1000.0, F(0.1))
    p = cap.default_pathing_params()
    assert (p.struct_size, p.validate, p.max_attach, p.max_length) == (32, 1, 1000.0, 10000.0)
    assert p.step == F(0.1) and p.pullback == F(0.1) and p.dist_divisor == 1000.0 and p.sound_speed == 343.0
    assert (cap.MAX_PATHING_PROBES, cap.MAX_PATHING_NODES, cap.MAX_PATHING_BATCH) == (1024, 16, 256)
    assert (cap.PATHING_FOUND, cap.PATHING_DIRECT, cap.PATHING_STALE, cap.PATHING_NO_PROBE, cap.PATHING_VOICE_KEY) == (1, 2, 4, NO_PROBE, KEY)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frequensee.h")).read()
    for name, value in (("FS_MAX_PATHING_PROBES", "1024"), ("FS_MAX_PATHING_NODES", "16"), ("FS_MAX_PATHING_BATCH", "256"), ("FS_PATHING_MIN_EDGE", "1.0f"),
                        ("FS_PATHING_MAX_LENGTH", "1048576.0f"), ("FS_PATHING_FOUND", "1u"), ("FS_PATHING_DIRECT", "2u"), ("FS_PATHING_STALE", "4u"),
                        ("FS_PATHING_NO_PROBE", "0xFFFFFFFFu"), ("FS_PATHING_VOICE_KEY", "0x80000003u")):
        assert f"#define {name} " in header and header.split(f"#define {name} ")[1].split()[0] == value
    assert cap.load().fs_abi_version() == 5, "the change only adds"
    assert KEY & 3 == 3 and KEY < 0xC0000000, "no diffraction key (edge <= 2), below the mixed keys"


NAMES = ("fs_pathing_set_probes", "fs_pathing_bake_params_default", "fs_pathing_bake", "fs_pathing_info", "fs_pathing_copy_graph",
         "fs_pathing_params_default", "fs_update_pathing_paths")


def test_exported_in_one_tier(pkg):
    contract.exported_in_one_tier(pkg, NAMES)


def test_null_context_and_no_device(pkg):
    cap = pkg._capi
    lib = cap.load()
    xyz = np.zeros((2, 3), np.float32)
    words = np.full(2, 7, np.uint32)
    before = words.tobytes()
    i32 = [C.c_int32(7) for _ in range(4)]
    assert lib.fs_pathing_set_probes(None, xyz.ctypes.data, 2) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_pathing_bake(None, None) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_pathing_info(None, *[C.byref(x) for x in i32]) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_pathing_copy_graph(None, words.ctypes.data, 2) == cap.ERR_INVALID_ARGUMENT
    lib.fs_pathing_bake_params_default(None)   # tolerated, like the other *_default calls
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        cfg = cap.default_config(num_bands=1)
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == cap.ERR_NO_DEVICE and h
        try:
            assert lib.fs_pathing_set_probes(h, xyz.ctypes.data, 2) == cap.ERR_NO_DEVICE
            assert b"no CPU fallback" in lib.fs_last_error(h)
            assert lib.fs_pathing_set_probes(h, xyz.ctypes.data, 1025) == cap.ERR_INVALID_ARGUMENT
            assert lib.fs_pathing_set_probes(h, xyz.ctypes.data, -1) == cap.ERR_INVALID_ARGUMENT
            assert lib.fs_pathing_bake(h, None) == cap.ERR_NO_DEVICE
            assert lib.fs_pathing_copy_graph(h, words.ctypes.data, 2) == cap.ERR_INVALID_ARGUMENT   # nothing baked
            assert lib.fs_pathing_copy_graph(h, None, 2) == cap.ERR_INVALID_ARGUMENT
            assert lib.fs_pathing_info(h, *[C.byref(x) for x in i32]) == cap.OK and [x.value for x in i32] == [0, 0, 0, 0]
            assert lib.fs_pathing_info(h, None, None, None, None) == cap.OK
        finally:
            lib.fs_context_destroy(h)
    assert words.tobytes() == before
    contract.null_context_and_no_device(pkg, QUERY)   # fs_pathing_params_default and fs_update_pathing_paths


def dijkstra64(y, dL):
    """float64: (distance, hops) from the listener to every probe over the restatement's graph and attach set, the legs' lengths
    from the float32 positions in double"""
    P = y.P.astype(np.float64)
    dist, hops = np.full(y.N, np.inf), np.zeros(y.N, np.int64)
    heap = []
    for k in range(y.N):
        if dL[k] < INF:
            heapq.heappush(heap, (float(np.linalg.norm(P[k] - y.L.astype(np.float64))), 1, k))
    while heap:
        dk, hk, k = heapq.heappop(heap)
        if dk >= dist[k]:
            continue
        dist[k], hops[k] = dk, hk
        for j in y.nbr[k]:
            heapq.heappush(heap, (dk + float(np.linalg.norm(P[j] - P[k])), hk + 1, int(j)))
    return dist, hops


def test_restatement_against_dijkstra(pkg, oracle_mod):
    """The restatement's d against a float64 Dijkstra on the same graph.  The bound, from the rule's roundings with u = 2^-24: a
    leg's length is sqrtf((ex ex + ey ey) + ez ez) of rounded differences — one rounding in each difference (relative u in e, 2 u
    in its square), one in each square, two additions (terms >= 0: relative errors do not grow), so the sum carries at most
    (2 + 1 + 2) u, its root half of that, and sqrtf adds u: 3.5 u per leg.  The route to a probe of h hops sums h legs with h - 1
    rounded additions, each at most u of a partial sum that is at most the length: (h - 1) u.  Together (h + 2.5) u to first order;
    the second-order terms, (h + 2.5)^2 u^2, stay below 0.5 u for h < 2 000.  fp32 d is the minimum over routes of the rounded sums
    (addition is monotone), so comparing each minimum with the other's route gives |d32 - d64| <= (h + 3) u d64 with h the larger of
    the two routes' hops.  max_length is out of the way (2^20)."""
    w, base = rooms_case(oracle_mod)
    y = Pathing(oracle_mod, w, room_probes())
    y.adj, y.nbr = base.adj, base.nbr
    y.listener(LIS, max_length=1048576.0)
    d64, h64 = dijkstra64(y, y.dL)
    h32 = np.zeros(y.N, np.int64)
    for k in range(y.N):
        q = k
        while y.d[k] < INF and q != LISTENER:
            h32[k] += 1
            q = int(y.pred[q])
    assert np.array_equal(np.isfinite(d64), y.d < INF) and np.isfinite(d64).sum() >= 25 and h32.max() >= 3
    for k in np.nonzero(np.isfinite(d64))[0]:
        assert abs(float(y.d[k]) - d64[k]) <= (max(h32[k], h64[k]) + 3) * U * d64[k], (k, y.d[k], d64[k])
    # the bound is not idle: some distance differs from the double's
    assert any(float(y.d[k]) != d64[k] for k in np.nonzero(np.isfinite(d64))[0])


def test_jacobi_and_in_place_relaxation_agree(pkg, oracle_mod):
    """the fixed point does not depend on the order of relaxation: Jacobi, in place ascending and in place descending give the same
    bits, with max_length out of the way and with max_length cutting routes off"""
    _, y = rooms_case(oracle_mod)
    for max_length in (10000.0, 700.0, 450.0):
        d, pred, rounds = y.relax(y.dL, max_length)
        assert rounds >= 2 or max_length < 500
        for order in ("inplace", "reversed"):
            d2, pred2, _ = y.relax(y.dL, max_length, order)
            assert np.array_equal(d.view(np.uint32), d2.view(np.uint32)) and np.array_equal(pred, pred2), (max_length, order)
    cut = y.relax(y.dL, 450.0)[0]
    assert np.any((cut == INF) & (y.d < INF)), "max_length = 450 cuts nothing off"


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def open_rooms(pkg, w, probes, L=LIS, fast=False, **bake):
    ctx = w.context(pkg, fast=fast)
    ctx.set_listener(L)
    ctx.pathing_set_probes(probes)
    edges = ctx.pathing_bake(**bake)
    return ctx, edges


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["sah", "device_morton"])
def test_three_rooms(pkg, oracle_mod, fast):
    w, y = rooms_case(oracle_mod)
    ctx, edges = open_rooms(pkg, w, room_probes(), fast=fast, **ROOMS_BAKE)
    assert edges == y.edges() and np.array_equal(graph_of(ctx), y.graph())
    assert ctx.pathing_info() == dict(probes=30, edges=edges, baked=True, scene_changed=False)
    pos = rooms_sources()
    h = place(ctx, pos)
    # only pathing answers SRC: no line of sight, no path round one edge, none round two parallel edges
    assert ctx.direct_paths(h[:1], samples=16, source_radius=20.0)[0]["visibility"] == 0
    assert ctx.diffraction_paths(h[:1])[0][0]["found"] == 0 and ctx.diffraction2_paths(h[:1], max_detour=1000.0)[0][0]["found"] == 0
    want = y.expect(pkg, pos)
    assert want[0]["flags"] == FOUND and want[0]["hops"] >= 3, "the far room is three probes away"
    assert np.count_nonzero(want["flags"] & FOUND) >= 60 and np.count_nonzero(want["flags"] & DIRECT) >= 10
    got = ctx.pathing_paths(h)
    assert_rows(got, want, "count 64")
    for i in range(64):
        assert ctx.pathing_paths(h[i:i + 1]).tobytes() == got[i:i + 1].tobytes(), f"row {i} alone"
    perm = np.random.default_rng(3).permutation(64)
    assert ctx.pathing_paths([h[i] for i in perm]).tobytes() == got[perm].tobytes()
    assert ctx.pathing_paths(h[7:12]).tobytes() == got[7:12].tobytes()
    ctx.close()


@functools.lru_cache(maxsize=None)
def scattered_case(oracle_mod, n):
    pts = np.random.default_rng(0x6A0 + n).uniform([20.0, 20.0, 20.0], [880.0, 380.0, 280.0], (n, 3)).astype(np.float32)
    return pts, Pathing(oracle_mod, three_rooms(), pts).bake(max_edge=400.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_graph_sizes(pkg, oracle_mod, n):
    """the word and the wave edges of a row"""
    pts, y = scattered_case(oracle_mod, n)
    ctx, edges = open_rooms(pkg, y.y.w, pts, max_edge=400.0)
    g = graph_of(ctx)
    assert g.shape == (n, (n + 31) // 32) and np.array_equal(g, y.graph()) and edges == y.edges()
    assert n < 63 or (edges > n and edges < n * (n - 1) // 2), "the graph is neither empty nor complete"
    y.listener(LIS)
    h = place(ctx, [SRC, LIS, [450.0, 200.0, 60.0]])
    assert_rows(ctx.pathing_paths(h), y.expect(pkg, [SRC, LIS, [450.0, 200.0, 60.0]]), f"N = {n}")
    ctx.close()


@pytest.mark.gpu
def test_graph_of_1024_probes(pkg, oracle_mod):
    """a lattice of 16 x 8 x 8 probes 35 cm apart across the door frame, max_edge = 63 cm: face, edge and body diagonals, at most
    26 neighbours; every word of the graph, and rows whose relaxation has a probe for every one of the workgroup's 1024 threads"""
    pts = np.array([[30.0 + 35.0 * i, 30.0 + 35.0 * j, 20.0 + 35.0 * k] for i in range(16) for j in range(8) for k in range(8)], np.float32)
    w = three_rooms()
    y = Pathing(oracle_mod, w, pts).bake(max_edge=63.0)
    assert y.adj.sum(axis=1).max() == 26 and y.adj.sum(axis=1).min() < 26
    ctx, edges = open_rooms(pkg, w, pts, max_edge=63.0)
    assert np.array_equal(graph_of(ctx), y.graph()) and edges == y.edges()
    y.listener(LIS, max_attach=120.0)
    pos = [[560.0, 250.0, 250.0], [580.0, 40.0, 30.0]]
    want = y.expect(pkg, pos, max_attach=120.0)
    assert np.all(want["flags"] == FOUND) and want["hops"].min() >= 4
    assert_rows(ctx.pathing_paths(place(ctx, pos), max_attach=120.0), want, "N = 1024")
    ctx.close()


CORRIDOR = dict(max_attach=35.0)


@pytest.mark.gpu
def test_corridor_of_200_probes(pkg, oracle_mod):
    """200 probes 10 cm apart in a line, max_edge = 15: only neighbours are linked; the listener attaches to probe 0 alone and the
    source to probe 199 alone, so d needs every one of the N rounds the loop is capped at and the path has more probes than a row
    reports"""
    w = World([(box([0.0, 0.0, 0.0], [2100.0, 100.0, 100.0], 1), WALLS, 1)], ALPHA, TAU, 4, SCAT)
    pts = np.array([[50.0 + 10.0 * k, 40.0, 60.0] for k in range(200)], np.float32)
    L, S = [20.0, 40.0, 60.0], [2070.0, 40.0, 60.0]
    y = Pathing(oracle_mod, w, pts).bake(max_edge=15.0).listener(L, **CORRIDOR)
    assert y.edges() == 199 and y.rounds == 199 and np.count_nonzero(y.dL < INF) == 1
    ctx, edges = open_rooms(pkg, w, pts, L=L, max_edge=15.0)
    assert edges == 199 and np.array_equal(graph_of(ctx), y.graph())
    h = place(ctx, [S])
    want = y.expect(pkg, [S], **CORRIDOR)
    assert want[0]["hops"] == 200 and want[0]["flags"] == FOUND | DIRECT and list(want[0]["probes"]) == list(range(16))
    assert (want[0]["first_probe"], want[0]["last_probe"]) == (0, 199)
    assert_rows(ctx.pathing_paths(h, **CORRIDOR), want, "corridor")
    # max_length cuts the route off half way: not FOUND, the row is zero but for distance and DIRECT
    short = dict(CORRIDOR, max_length=1000.0)
    want = y.listener(L, **short).expect(pkg, [S], **short)
    assert want[0]["flags"] == DIRECT and want[0]["distance"] == 2050.0 and want[0]["length"] == 0
    assert_rows(ctx.pathing_paths(h, **short), want, "corridor, max_length 1000")
    ctx.close()


@pytest.mark.gpu
def test_ties(pkg, oracle_mod):
    """a slab in the middle of a square room, the listener and the sources on its axis: the routes either side are equal to the
    bit, at the source (two probes with one total) and inside the graph (two neighbours with one c); the smaller index wins"""
    w = World([(box([0.0, 0.0, 0.0], [600.0, 600.0, 300.0], 1), WALLS, 1),
               (quad_grid((300.0, 200.0, 0.0), (0.0, 200.0, 0.0), (0.0, 0.0, 300.0), 1), OPAQUE, 2)], ALPHA, TAU, 4, SCAT)
    pts = np.array([[300.0, 500.0, Z], [300.0, 100.0, Z], [450.0, 300.0, Z]], np.float32)
    L, near, far = [100.0, 300.0, Z], [520.0, 300.0, Z], [580.0, 300.0, Z]
    params = dict(max_attach=300.0)
    y = Pathing(oracle_mod, w, pts).bake(max_edge=350.0).listener(L, **params)
    assert y.edges() == 2 and y.dL[2] == INF and bits(y.dL[0]) == bits(y.dL[1])
    assert bits(F(y.d[0] + y.w[0, 2])) == bits(F(y.d[1] + y.w[1, 2])) == bits(y.d[2]) and y.pred[2] == 0
    _, totals = y.row(near, **params)
    assert bits(totals[0]) == bits(totals[1]) and bits(totals[0]) < bits(totals[2])
    want = y.expect(pkg, [near, far], **params)
    assert list(want["last_probe"]) == [0, 2] and list(want["first_probe"]) == [0, 0] and list(want["hops"]) == [1, 2]
    ctx, _ = open_rooms(pkg, w, pts, L=L, max_edge=350.0)
    assert np.array_equal(graph_of(ctx), y.graph())
    assert_rows(ctx.pathing_paths(place(ctx, [near, far]), **params), want, "ties")
    ctx.close()


CELL_LO, CELL_HI = [470.0, 470.0, 70.0], [530.0, 530.0, 130.0]


def cell_world(actor):
    return World([(box([0.0, 0.0, 0.0], [600.0, 600.0, 300.0], 1), WALLS, 1), (box(CELL_LO, CELL_HI, 1), OPAQUE, actor)], ALPHA, TAU, 4, SCAT)


@pytest.mark.gpu
def test_degenerate_cases(pkg, oracle_mod):
    """the listener exactly on a probe, a source exactly on a probe, two probes closer than FS_PATHING_MIN_EDGE, a source in a closed
    cell, DIRECT in an open room"""
    w = cell_world(2)
    pts = np.array([[100.0, 100.0, 100.0], [100.5, 100.0, 100.0], [300.0, 100.0, 100.0]], np.float32)
    L = [100.0, 100.0, 100.0]
    pos = [[300.0, 100.0, 100.0], [200.0, 250.0, 90.0], [497.0, 506.0, 95.0], L]
    y = Pathing(oracle_mod, w, pts).bake()
    assert y.edges() == 2 and not y.adj[0, 1] and y.adj[0, 2] and y.adj[1, 2]
    ctx, edges = open_rooms(pkg, w, pts, L=L)
    assert edges == 2 and np.array_equal(graph_of(ctx), y.graph())
    h = place(ctx, pos)
    for params in (dict(), dict(max_attach=150.0)):   # the far probe attached to the listener, and reached through the probe it stands on
        y.listener(L, **params)
        want = y.expect(pkg, pos, **params)
        assert y.dL[0] == 0 and want[0]["flags"] == FOUND | DIRECT and want[0]["last_probe"] == (2 if params else 0)   # (a tie: probe 0 at 200, probe 2 at 0)
        assert want[0]["hops"] == (2 if params else 1) and want[0]["length"] == 200.0 and want[0]["detour"] == 0.0
        assert np.array_equal(want[0]["direction"], [1.0, 0.0, 0.0]) and np.array_equal(want[0]["departure"], [-1.0, 0.0, 0.0])
        assert want[2]["flags"] == 0 and want[2]["distance"] > 0 and want[2].tobytes().count(b"\0") >= 148   # the closed cell
        assert want[3]["flags"] == FOUND | DIRECT and want[3]["length"] == 0 and want[3]["hops"] == 1 and want[3]["distance"] == 0
        assert_rows(ctx.pathing_paths(h, **params), want, f"degenerate {params}")
    ctx.close()


@pytest.mark.gpu
def test_own_actors(pkg, oracle_mod):
    """a source inside its registered mesh attaches through it, a listener inside its own likewise; the bake knows no actors: a
    probe pair either side of the mesh has no edge"""
    w = cell_world(7)
    pts = np.array([[400.0, 500.0, 100.0], [590.0, 500.0, 100.0], [300.0, 300.0, 100.0]], np.float32)
    inside, L = [497.0, 506.0, 95.0], [100.0, 100.0, 100.0]
    y = Pathing(oracle_mod, w, pts).bake()
    assert not y.adj[0, 1] and y.adj[0, 2] and y.adj[1, 2]
    ctx, _ = open_rooms(pkg, w, pts, L=L)
    assert np.array_equal(graph_of(ctx), y.graph())
    h = place(ctx, [inside, inside])
    ctx.set_source_object(h[0], 7)
    y.listener(L)
    want = y.expect(pkg, [inside, inside], src_obj=[7, NO_OBJECT])
    assert want[0]["flags"] == FOUND | DIRECT and want[1]["flags"] == 0
    assert_rows(ctx.pathing_paths(h), want, "source in its mesh")
    ctx.set_listener(inside)
    ctx.set_listener_object(7)
    ctx.set_source_position(h[1], L)
    y.listener(inside, lo=7)
    want = y.expect(pkg, [inside, L], src_obj=[7, NO_OBJECT])
    assert np.all(want["flags"] == FOUND | DIRECT)
    assert_rows(ctx.pathing_paths(h), want, "listener in its mesh")
    y.listener(inside, lo=NO_OBJECT)
    ctx.set_listener_object()
    want = y.expect(pkg, [inside, L], src_obj=[7, NO_OBJECT])
    assert want[1]["flags"] == 0 and np.all(y.dL == INF)
    assert_rows(ctx.pathing_paths(h), want, "listener shut in")
    ctx.close()


DOOR_LIS = [150.0, 350.0, Z]
DOOR_PARAMS = dict(max_attach=200.0)


@pytest.mark.gpu
def test_door(pkg, oracle_mod):
    w = three_rooms(door=True)
    shut = w.tri.copy()
    idx = w.obj == DOOR_ACTOR
    p = shut[idx]
    shut[idx] = np.stack([((SHUT[k, 0] * p[..., 0] + SHUT[k, 1] * p[..., 1]) + SHUT[k, 2] * p[..., 2]) + SHUT[k, 3] for k in range(3)], axis=-1)
    pts = room_probes()
    y_open = Pathing(oracle_mod, w, pts).bake(**ROOMS_BAKE).listener(DOOR_LIS, **DOOR_PARAMS)
    first = y_open.expect(pkg, [SRC], **DOOR_PARAMS)
    assert first[0]["flags"] == FOUND and first[0]["hops"] >= 3 and np.count_nonzero(y_open.dL < INF) == 6, "the listener attaches in its own room only"
    ctx, _ = open_rooms(pkg, w, pts, L=DOOR_LIS, **ROOMS_BAKE)
    h = place(ctx, [SRC])
    assert_rows(ctx.pathing_paths(h, **DOOR_PARAMS), first, "door open")
    assert not ctx.pathing_info()["scene_changed"]
    ctx.set_object_transforms([DOOR_ACTOR], SHUT[None])
    assert ctx.pathing_info()["scene_changed"] and ctx.pathing_info()["baked"]
    # the old graph over the new triangles: the same route, STALE if it is looked at again (the call refits first)
    y_stale = Pathing(oracle_mod, w, pts, shut)
    y_stale.adj, y_stale.nbr = y_open.adj, y_open.nbr
    y_stale.listener(DOOR_LIS, **DOOR_PARAMS)
    want = y_stale.expect(pkg, [SRC], **DOOR_PARAMS)
    assert want[0]["flags"] == FOUND | STALE and want[0]["length"] == first[0]["length"]
    assert_rows(ctx.pathing_paths(h, **DOOR_PARAMS), want, "door shut, validate")
    blind = dict(DOOR_PARAMS, validate=0)
    want = y_stale.expect(pkg, [SRC], **blind)
    assert want[0]["flags"] == FOUND
    assert_rows(ctx.pathing_paths(h, **blind), want, "door shut, validate = 0")
    # baked again: the frame is the only way through
    edges = ctx.pathing_bake(**ROOMS_BAKE)
    y_shut = Pathing(oracle_mod, w, pts, shut).bake(**ROOMS_BAKE).listener(DOOR_LIS, **DOOR_PARAMS)
    assert edges == y_shut.edges() < y_open.edges() and np.array_equal(graph_of(ctx), y_shut.graph())
    assert not ctx.pathing_info()["scene_changed"]
    want = y_shut.expect(pkg, [SRC], **DOOR_PARAMS)
    assert want[0]["flags"] == 0
    assert_rows(ctx.pathing_paths(h, **DOOR_PARAMS), want, "door shut, baked again")
    # the door back and a new bake: the first answer
    ctx.set_object_transforms([DOOR_ACTOR], REST[None])
    assert ctx.pathing_info()["scene_changed"]
    assert ctx.pathing_bake(**ROOMS_BAKE) == y_open.edges() and np.array_equal(graph_of(ctx), y_open.graph())
    assert ctx.pathing_paths(h, **DOOR_PARAMS).tobytes() == first.tobytes()
    for change in (lambda: ctx.update_triangles(0, w.tri[:1]), ctx.refit, lambda: ctx.set_scene(w.tri, w.mat, w.absorption, w.transmission, w.scattering,
                                                                                                   object_ids=w.obj)):
        assert not ctx.pathing_info()["scene_changed"]
        change()
        assert ctx.pathing_info()["scene_changed"]
        ctx.pathing_bake(**ROOMS_BAKE)
    assert ctx.pathing_paths(h, **DOOR_PARAMS).tobytes() == first.tobytes()
    ctx.close()


inf, nan = float("inf"), float("nan")
QUERY = contract.Query(
    kind="pathing", dtypes=("PATHING_DTYPE",), world=three_rooms, src=SRC, lis=LIS, wrong_struct_size=28,
    refused=(dict(validate=2), dict(validate=-1), dict(max_attach=0.0), dict(max_attach=-1.0), dict(max_attach=nan), dict(max_attach=inf),
             dict(max_length=0.0), dict(max_length=-1.0), dict(max_length=nan), dict(max_length=inf), dict(max_length=1048577.0), dict(step=-0.1),
             dict(step=nan), dict(step=inf), dict(pullback=-1.0), dict(pullback=nan), dict(pullback=inf), dict(dist_divisor=0.0),
             dict(dist_divisor=-1.0), dict(dist_divisor=nan), dict(dist_divisor=inf), dict(sound_speed=0.0), dict(sound_speed=-1.0),
             dict(sound_speed=nan), dict(sound_speed=inf)),
    fewer=dict(validate=0))


@pytest.mark.gpu
def test_errors_and_untouched_state(pkg, oracle_mod):
    cap = pkg._capi
    lib = cap.load()
    _, y = rooms_case(oracle_mod)
    pts = room_probes()
    call = contract.Calls(pkg, QUERY)
    ctx, src, out = call.ctx, call.src, call.bufs[0]
    twin = pkg.Context(num_bands=4)   # never sees a refused call
    tsrc = twin.create_source(SRC)
    words = np.full(30, 7, np.uint32)
    sentinel = words.tobytes()

    def bake(**kw):
        return lib.fs_pathing_bake(ctx.h, C.byref(cap.default_pathing_bake_params(**dict(ROOMS_BAKE, **kw))))

    def same_as_twin(where):
        assert ctx.pathing_info() == twin.pathing_info(), where
        if twin.pathing_info()["baked"]:
            assert np.array_equal(ctx.pathing_graph(), twin.pathing_graph()), where
            assert ctx.pathing_paths([src, src]).tobytes() == twin.pathing_paths([tsrc, tsrc]).tobytes(), where

    bad_pts = pts.copy()
    bad_pts[17, 1] = nan
    assert bake() == cap.ERR_INVALID_ARGUMENT                                       # no probes
    assert lib.fs_pathing_set_probes(ctx.h, bad_pts.ctypes.data, 30) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_pathing_set_probes(ctx.h, pts.ctypes.data, 1025) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_pathing_set_probes(ctx.h, pts.ctypes.data, -1) == cap.ERR_INVALID_ARGUMENT
    same_as_twin("refused probes")
    for c in (ctx, twin):
        c.pathing_set_probes(pts)
    assert bake() == cap.ERR_NOT_COMMITTED and call() == cap.ERR_INVALID_ARGUMENT   # (nothing baked)
    for c in (ctx, twin):
        call.commit(c)
    assert call() == cap.ERR_INVALID_ARGUMENT and lib.fs_pathing_copy_graph(ctx.h, words.ctypes.data, 30) == cap.ERR_INVALID_ARGUMENT
    for kw in (dict(max_edge=0.0), dict(max_edge=-1.0), dict(max_edge=nan), dict(max_edge=inf), dict(step=-0.1), dict(step=nan), dict(step=inf)):
        assert bake(**kw) == cap.ERR_INVALID_ARGUMENT, kw
    q = cap.default_pathing_bake_params()
    q.struct_size = 8
    assert lib.fs_pathing_bake(ctx.h, C.byref(q)) == cap.ERR_INVALID_ARGUMENT
    same_as_twin("refused bakes")
    assert bake() == cap.OK and twin.pathing_bake(**ROOMS_BAKE) == y.edges()
    call.refusals()
    for n in (29, 31, 0, -1):
        assert lib.fs_pathing_copy_graph(ctx.h, words.ctypes.data, n) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_pathing_copy_graph(ctx.h, None, 30) == cap.ERR_INVALID_ARGUMENT
    assert words.tobytes() == sentinel, "a refused call wrote"
    call.unwritten()
    same_as_twin("refused updates")
    # NULL params = the defaults; one handle twice; extreme but legal values are taken
    assert_rows(call.null_params_are_the_defaults()[0], y.expect(pkg, [SRC, SRC]), "defaults, one handle twice")
    assert call(max_length=1048576.0, step=0.0, pullback=0.0, validate=0) == cap.OK and out[0]["flags"] == FOUND
    assert lib.fs_pathing_bake(ctx.h, None) == cap.OK and ctx.pathing_info()["edges"] > y.edges()
    # new probes drop the bake; clearing them too
    ctx.pathing_set_probes(pts[:5])
    assert ctx.pathing_info() == dict(probes=5, edges=0, baked=False, scene_changed=False)
    assert call() == cap.ERR_INVALID_ARGUMENT and lib.fs_pathing_copy_graph(ctx.h, words.ctypes.data, 5) == cap.ERR_INVALID_ARGUMENT
    ctx.pathing_set_probes(None)
    assert ctx.pathing_info()["probes"] == 0 and bake() == cap.ERR_INVALID_ARGUMENT
    ctx.pathing_set_probes(pts)
    assert bake() == cap.OK
    same_as_twin("set again")

    # a successful call leaves the sources alone: energy, IR publish number, occlusion scalar
    def query():
        ctx.pathing_bake(**ROOMS_BAKE)
        assert ctx.pathing_paths([src])[0]["flags"] == FOUND

    contract.leaves_sources_alone(pkg, ctx, src, query)
    ctx.close()
    twin.close()
    # an empty committed scene: every pair within max_edge is an edge, every line is free
    e = World([], ALPHA, TAU, 4, SCAT)
    ye = Pathing(oracle_mod, e, pts).bake(**ROOMS_BAKE).listener(LIS)
    ctx, edges = open_rooms(pkg, e, pts, **ROOMS_BAKE)
    assert edges == ye.edges() and np.array_equal(graph_of(ctx), ye.graph())
    assert_rows(ctx.pathing_paths(place(ctx, [SRC, LIS])), ye.expect(pkg, [SRC, LIS]), "empty scene")
    ctx.close()


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg, oracle_mod):
    w, _ = rooms_case(oracle_mod)
    ctx, _ = open_rooms(pkg, w, room_probes(), **ROOMS_BAKE)
    h = place(ctx, rooms_sources()[:40])
    graph = graph_of(ctx)

    def churn(ctx):
        ctx.pathing_bake(**ROOMS_BAKE)
        ctx.pathing_set_probes(room_probes()[::-1])
        ctx.pathing_bake(**ROOMS_BAKE)
        ctx.pathing_set_probes(room_probes())
        ctx.pathing_bake(**ROOMS_BAKE)

    def found(ctx, h, first, fewer):
        assert np.array_equal(graph_of(ctx), graph) and ctx.pathing_paths(h).tobytes() == first[0].tobytes()
        assert np.any(first[0]["flags"] & FOUND) and not np.any(first[0]["flags"] & STALE)

    contract.steady_state_allocates_nothing(pkg, QUERY, opened=(ctx, h), churn=churn, found=found)


@pytest.mark.gpu
def test_queries_interleaved_on_one_context(pkg, oracle_mod):
    """pathing shares the chain and the staging code with the other queries but no buffer: between calls of the other five, with
    counts that use, grow and reuse every staging, each call returns the bytes it returns on a fresh context"""
    w, _ = rooms_case(oracle_mod)
    pos = rooms_sources()[:33]

    def fresh():
        ctx, _ = open_rooms(pkg, w, room_probes(), **ROOMS_BAKE)
        return ctx, place(ctx, pos)

    kinds = ("pathing", "mixed", "diffraction2", "reflection2", "pathing", "reflection", "diffraction", "direct", "pathing")
    calls = [(k, 5) for k in kinds] + [(k, 33) for k in reversed(kinds)] + [(k, 5) for k in kinds]
    got = contract.queries_interleaved_on_one_context(fresh, calls, dict(mixed=dict(max_length=1000.0), diffraction2=dict(max_detour=1000.0)))
    # the comparison is not of zeros
    by = {c: g for c, g in zip(calls, got)}
    assert np.any(got[0][0]["flags"] & FOUND)
    assert np.any(by["reflection2", 33][0]["returned"] > 0) and np.any(by["reflection", 33][0]["returned"] > 0)
    assert np.any(by["diffraction", 33][0]["returned"] > 0) and np.any(by["diffraction2", 33][0]["near"] > 0)


@pytest.mark.gpu
def test_component_layer(pkg, oracle_mod):
    """Voices(pathing=) of the reflection, the binaural and the ambisonic plugin: one voice for a FOUND row that is not DIRECT, none
    for a source in plain sight; its key is the one no other kind has"""
    from test_direct_render import noise
    w, y = rooms_case(oracle_mod)
    frame, taps = 64, 15
    sub = pkg.AudioRayTracingSubsystem(num_bands=4)
    sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
    sub.SetMaterials(w.absorption, w.transmission, w.scattering)
    comp = pkg.FrequenSeeAudioComponent(SRC)
    comp.OnRegister(sub)
    sub.SetListenerLocation(LIS)
    assert sub.SetPathingProbes(room_probes(), **ROOMS_BAKE) == y.edges() and sub.PathingInfo()["baked"]
    plug = pkg.FrequenSeeAudioReflectionPlugin(sub)
    plug.Initialize(frame, taps, 32, 0.05)
    plug.OnInitSource(comp)
    latency = ((taps - 1) // 2) / sub.ctx.cfg.sample_rate
    right, forward = [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]
    rng = np.random.default_rng(5)
    started = []
    for pos, heard in ((SRC, True), (SRC, True), ([200.0, 300.0, Z], False)):
        comp.SetComponentLocation(pos)
        rows, paths = sub.UpdateReflectionPaths(max_paths=8)
        drows, dpaths = sub.UpdateDiffractionPaths()
        prow = sub.UpdatePathingPaths()
        assert_rows(prow, y.expect(pkg, [pos]), "component layer")
        assert bool(prow[0]["flags"] & FOUND) and bool(prow[0]["flags"] & DIRECT) != heard
        base = plug.Voices(rows[0], paths[0], right=right, diffraction=(drows[0], dpaths[0]))
        voices = plug.Voices(rows[0], paths[0], right=right, diffraction=(drows[0], dpaths[0]), pathing=prow[0])
        assert np.array_equal(voices[:len(base)], base) and len(voices) == len(base) + (1 if heard else 0)
        assert KEY not in [int(k) for k in base["key"]]
        if heard:
            v = voices[-1]
            assert int(v["key"]) == KEY
            assert np.array_equal(v["band_gain"], prow[0]["gain"]) and np.all(prow[0]["gain"][:4] > 0)
            assert float(v["delay"]) == pytest.approx(float(prow[0]["delay"]) - latency, abs=1e-7)
            t = (float(np.dot(prow[0]["direction"].astype(np.float64), right)) + 1.0) * np.pi / 4.0
            assert np.allclose(v["channel_gain"], [np.cos(t), np.sin(t)], atol=1e-6)
            for cls in (pkg.FrequenSeeAudioBinauralPlugin, pkg.FrequenSeeAudioAmbisonicPlugin):
                b = cls(sub).Voices(rows[0], paths[0], forward, right, diffraction=(drows[0], dpaths[0]), pathing=prow[0])
                assert int(b[-1]["key"]) == KEY and np.array_equal(b[-1]["band_gain"], prow[0]["gain"])
                assert np.allclose(b[-1]["direction"], prow[0]["direction"], atol=1e-6) and len(b) == len(voices)
        out, counts = plug.ProcessAudio([comp], noise(rng, 1, frame), rows, paths, right=right, diffraction=(drows, dpaths), pathing=prow)
        assert int(counts[0]["dropped"]) == 0
        started.append(int(counts[0]["started"]))
    assert started[0] >= 1 and started[1] == 0, "a steady source starts nothing"
    plug.OnReleaseSource(comp)
    sub.Deinitialize()
