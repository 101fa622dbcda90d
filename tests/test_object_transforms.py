"""fs_scene_set_object_transforms: registered actors moved by a 3 x 4 matrix applied to their rest triangles.

Method: context A uses the new call; context B gets the numpy float32 restatement of the header's arithmetic
(x' = ((r00 x + r01 y) + r02 z) + tx, every operation rounded) through fs_scene_update_triangles.  The header promises
that both leave the same committed scene bit for bit, before and after the refit, so every comparison here is on bytes:
the arrays fs_debug_scene_snapshot exposes (tests/tree_check.py), traced rays, deterministic frames and published IRs.
tree_check's restatements of the records and of the refit are a second opinion on A alone.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_check as tc  # noqa: E402

T = 1500
ABSORPTION = np.array([[0.3], [0.5], [0.8]], np.float32)
# object id -> triangles it owns: the wave (64) and workgroup (256) boundaries of the kernel's per-object search, and one
# large rest.  Ids are neither dense nor sorted; 13 and 20 are interleaved in input order, the others are contiguous runs.
SIZES = {7: 1, 11: 63, 12: 64, 13: 65, 20: 257, 900: T - (1 + 63 + 64 + 65 + 257)}
ARRAYS = tuple(k for k in tc.WHAT if k != "header")


def xf(m, p):
    """the header's arithmetic on float32 arrays: m [12] or [3][4] row-major, p [..., 3] -> [..., 3]"""
    m = np.asarray(m, np.float32).reshape(3, 4)
    p = np.asarray(p, np.float32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    out = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)]
    assert all(o.dtype == np.float32 for o in out)
    return np.stack(out, axis=-1)


def rotation(axis, angle, t=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.concatenate([R @ np.diag(scale), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(np.float32)


IDENTITY = rotation((0, 0, 1), 0.0)


def make_scene(seed=5):
    rng = np.random.default_rng(seed)
    tri = tc.soup("mixed", T, rng)
    mat = rng.integers(0, 3, T).astype(np.uint16)
    obj = np.empty(T, np.uint32)
    at = 0
    for k in (7, 11, 12):
        obj[at:at + SIZES[k]] = k; at += SIZES[k]
    n = SIZES[13] + SIZES[20]
    mix = np.full(n, 20, np.uint32)
    mix[rng.permutation(n)[:SIZES[13]]] = 13
    obj[at:at + n] = mix; at += n
    obj[at:] = 900
    assert {int(k): int((obj == k).sum()) for k in SIZES} == SIZES
    assert np.any(np.diff(np.nonzero(obj == 13)[0]) > 1) and np.any(np.diff(np.nonzero(obj == 20)[0]) > 1)
    return tri, mat, obj


def runs(idx):
    """sorted indices -> [(first, count)] of its contiguous runs"""
    cut = np.nonzero(np.diff(idx) != 1)[0] + 1
    return [(int(r[0]), int(r.shape[0])) for r in np.split(idx, cut)]


class Pair:
    """A: the new call.  B: the restatement through update_triangles.  rest / cur: the positions both must hold."""

    def __init__(self, pkg, fast=False, seed=5, pipelining=0):
        self.tri, self.mat, self.obj = make_scene(seed)
        self.rest, self.cur = self.tri.copy(), self.tri.copy()
        self.a, self.b = pkg.Context(num_bands=1), pkg.Context(num_bands=1)
        for c in (self.a, self.b):
            if pipelining:
                c.set_pipelining(pipelining)
            c.set_scene(self.tri, self.mat, ABSORPTION, object_ids=self.obj, fast=fast)

    def transform(self, ids, mats):
        mats = np.asarray(mats, np.float32).reshape(len(ids), 3, 4)
        self.a.set_object_transforms(ids, mats)
        for k, m in zip(ids, mats):
            idx = np.nonzero(self.obj == k)[0]
            self.cur[idx] = xf(m, self.rest[idx])
            for first, count in runs(idx):
                self.b.update_triangles(first, self.cur[first:first + count])

    def update(self, first, tris):
        tris = np.asarray(tris, np.float32)
        for c in (self.a, self.b):
            c.update_triangles(first, tris)
        self.rest[first:first + tris.shape[0]] = tris
        self.cur[first:first + tris.shape[0]] = tris

    def each(self, fn):
        return fn(self.a), fn(self.b)

    def close(self):
        self.a.close(); self.b.close()


def same(sa, sb, names, where):
    for k in names:
        x, y = getattr(sa, k), getattr(sb, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{where}: {k} differs"


def compare_pending(p, nodes_before, where):
    """after the call, before the refit: records new and equal, A's boxes still the old ones"""
    sa, sb = p.each(tc.snapshot)
    same(sa, sb, ("tri64", "tri48", "nrm"), where)
    assert sa.header["refit_pending"] == 1 and sb.header["refit_pending"] == 1, where
    assert sa.nodes.tobytes() == nodes_before, f"{where}: the call itself changed the boxes"
    return sa


def compare_refitted(p, where):
    """after fs_scene_refit: every array and the header, amax and padding included; then the second opinion on A"""
    p.each(lambda c: c.refit())
    sa, sb = p.each(tc.snapshot)
    same(sa, sb, ARRAYS, where)
    assert sa.header == sb.header, (where, sa.header, sb.header)
    assert sa.header["refit_pending"] == 0
    found = tc.check_records(sa, p.cur, p.mat, p.obj) + tc.check_refit(sa)
    assert found == [], where + "\n" + "\n".join(found)
    return sa


def rays(seed, cur, n=400):
    """half of the rays aimed at triangles of the scene as it stands (area or not), half anywhere"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-2500, 2500, (n, 3))
    d = rng.normal(size=(n, 3))
    aim = cur[rng.integers(0, cur.shape[0], n // 2)].astype(np.float64).mean(axis=1)
    d[:n // 2] = aim - o[:n // 2]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def compare_traces(p, pkg, src, seed, where):
    """400 random rays, closest hit and any hit, and one deterministic frame: identical in A and B"""
    o, d = rays(seed, p.cur)
    for any_hit in (0, 1):
        ra, rb = p.each(lambda c: c.trace_rays(o, d, 1e6, any_hit=any_hit))
        for x, y, what in zip(ra, rb, ("hit", "t", "tri", "normal")):
            assert x.tobytes() == y.tobytes(), f"{where}: {what} differs (any_hit = {any_hit})"
        if any_hit == 0:
            assert ra[0].sum() >= o.shape[0] // 4, f"{where}: half of the rays are aimed at triangles, {ra[0].sum()} hit"
    prm = pkg.default_params(num_rays=8192, depth=8, seed=seed, flags=pkg._capi.FLAG_DETERMINISTIC)
    ea = p.a.compute_energy_response(src[0], prm)
    eb = p.b.compute_energy_response(src[1], prm)
    assert ea.tobytes() == eb.tobytes(), f"{where}: the deterministic frame differs"
    assert ea.any(), f"{where}: the frame deposited nothing"
    return ea


def add_sources(p):
    for c in (p.a, p.b):
        c.set_listener((150.0, -100.0, 60.0))
    return p.each(lambda c: c.create_source((-300.0, 200.0, 40.0)))


# ---- 1: records and boxes ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("build", ["commit", "commit_fast"])
def test_records_and_boxes_equal_the_update_route(pkg, build):
    p = Pair(pkg, fast=build == "commit_fast")
    rng = np.random.default_rng(17)
    every = [int(k) for k in rng.permutation(list(SIZES))]
    oblique = [rotation((1.0, 2.0, -0.5), 0.3 + 0.37 * i, t=(40.0 * i - 90.0, 25.0, -13.5 * i)) for i in range(len(every))]
    far = rotation((0, 0, 1), 0.0, t=(52000.0, 0.0, 0.0))
    steps = [("a translation, one object", [20], [rotation((0, 0, 1), 0.0, t=(130.0, -75.5, 21.25))]),
             ("oblique rotations, every object in shuffled order", every, oblique),
             ("non-uniform scale with a mirror", [13, 12, 11, 7],
              [rotation((0, 1, 0), 0.0, t=(5.0, 0.0, -8.0), scale=(-1.5, 0.75, 2.0))] * 4),
             ("far outside the committed bounds", [11], [far]),
             ("back by the identity", [11], [IDENTITY])]
    assert np.linalg.det(np.asarray(steps[2][2][0], np.float64)[:, :3]) < 0
    nodes = tc.fetch(p.a, "nodes").tobytes()
    amax_before = None
    for where, ids, mats in steps:
        p.transform(ids, mats)
        compare_pending(p, nodes, where)
        sa = compare_refitted(p, where)
        nodes = sa.nodes.tobytes()
        if where.startswith("far"):
            assert sa.header["amax"] > 52000.0 and tc.refit_pad(sa.header) > np.float32(0.15)
            amax_before = sa.header["amax"]
        if where.startswith("back"):
            assert sa.header["amax"] == amax_before             # the padding never shrinks between commits
            idx = np.nonzero(p.obj == 11)[0]
            assert np.array_equal(p.cur[idx], p.rest[idx])      # the identity: the rest positions as numbers
    p.close()


# ---- 2: absolute, not cumulative ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_absolute_not_cumulative(pkg):
    m1 = rotation((0.3, -1.0, 0.8), 1.1, t=(200.0, 10.0, -40.0))
    m2 = rotation((1.0, 0.2, 0.1), -0.6, t=(-35.0, 80.0, 12.0), scale=(1.0, 1.25, 0.5))
    tri, mat, obj = make_scene()
    one, two = pkg.Context(num_bands=1), pkg.Context(num_bands=1)
    for c in (one, two):
        c.set_scene(tri, mat, ABSORPTION, object_ids=obj)
    one.set_object_transform(20, m1)
    one.set_object_transform(20, m2)
    two.set_object_transform(20, m2)
    sa, sb = tc.snapshot(one), tc.snapshot(two)
    same(sa, sb, ("tri64", "tri48", "nrm"), "M1 then M2 against M2 alone")
    one.refit(); two.refit()
    sa, sb = tc.snapshot(one), tc.snapshot(two)
    same(sa, sb, ("nodes", "tri64", "tri48", "nrm", "coop4", "coop16"), "M1 then M2 against M2 alone, refitted")
    idx = np.nonzero(obj == 20)[0]
    cur = tri.copy(); cur[idx] = xf(m2, tri[idx])
    assert tc.check_records(sa, cur, mat, obj) == []
    one.close(); two.close()


# ---- 3: mixed with fs_scene_update_triangles --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_with_update_triangles(pkg):
    p = Pair(pkg)
    rng = np.random.default_rng(23)
    first = int(np.nonzero(p.obj == 900)[0][0]) + 100            # 40 triangles of the large object
    assert np.all(p.obj[first:first + 40] == 900)
    m1 = rotation((0.0, 1.0, 1.0), 0.8, t=(60.0, -20.0, 33.0))
    nodes = tc.fetch(p.a, "nodes").tobytes()
    p.transform([900], [m1])
    nodes = compare_refitted(p, "first transform").nodes.tobytes()
    p.update(first, tc.soup("uniform", 40, rng, offset=(300.0, 300.0, -100.0)))
    compare_pending(p, nodes, "40 triangles rewritten")
    nodes = compare_refitted(p, "40 triangles rewritten").nodes.tobytes()
    m2 = rotation((1.0, 0.0, 0.3), -1.2, t=(-80.0, 15.0, 5.0), scale=(0.9, 1.1, 1.0))
    p.transform([900], [m2])                                     # the 40 start from their new rest positions
    assert np.array_equal(p.cur[first:first + 40], xf(m2, p.rest[first:first + 40]))
    compare_pending(p, nodes, "second transform")
    compare_refitted(p, "second transform")
    p.close()


# ---- 4: traces, frames, later commits -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_traces_frames_and_later_commits(pkg):
    p = Pair(pkg)
    src = add_sources(p)
    before = compare_traces(p, pkg, src, 31, "before any transform")
    p.transform([20, 900], [rotation((0.2, 0.1, 1.0), 0.5, t=(90.0, -60.0, 10.0)), rotation((1.0, 1.0, 0.0), 0.25, t=(0.0, 45.0, -20.0))])
    moved = compare_traces(p, pkg, src, 31, "after a transform")       # (the pending refit runs before the trace)
    assert moved.tobytes() != before.tobytes()
    for c in (p.a, p.b):                                                 # no new triangles: the commit builds over the world positions
        c.check(c.lib.fs_scene_commit(c.h))
    sa, sb = p.each(tc.snapshot)
    same(sa, sb, ARRAYS, "after a second commit")
    assert sa.header == sb.header
    assert tc.check_records(sa, p.cur, p.mat, p.obj) == []
    again = compare_traces(p, pkg, src, 31, "after a second commit")
    assert again.tobytes() == moved.tobytes()                            # results do not depend on the tree
    p.transform([900, 13], [rotation((0.0, 0.0, 1.0), -0.7, t=(10.0, 10.0, 10.0)), IDENTITY])   # still maps the REST pose
    idx = np.nonzero(p.obj == 13)[0]
    assert np.array_equal(p.cur[idx], p.tri[idx])
    compare_traces(p, pkg, src, 32, "a transform after the second commit")
    compare_refitted(p, "a transform after the second commit")
    p.close()


# ---- 5: progressive commit ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_transform_during_a_progressive_commit(pkg):
    p = Pair(pkg, fast="progressive")
    src = add_sources(p)
    assert p.a.refine_pending() and p.b.refine_pending()       # the swap happens at a trace or at refine_wait, not before
    p.transform([12, 20], [rotation((1.0, 0.5, 0.2), 0.9, t=(-120.0, 30.0, 55.0)), rotation((0.0, 1.0, 0.0), 0.4, t=(15.0, 0.0, -70.0))])
    assert p.a.refine_pending()
    p.each(lambda c: c.refine_wait())
    assert not p.a.refine_pending() and tc.fetch(p.a, "header")["fast"] == 0
    compare_traces(p, pkg, src, 41, "after the swap")
    sa = compare_refitted(p, "after the swap")
    assert tc.check_records(sa, p.cur, p.mat, p.obj) == []
    p.transform([12], [rotation((0.0, 0.0, 1.0), 0.2, t=(1.0, 2.0, 3.0))])      # the swap kept the rest pose
    compare_traces(p, pkg, src, 42, "a transform after the swap")
    compare_refitted(p, "a transform after the swap")
    p.close()


# ---- 6: pipelined stream -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_transform_between_pipelined_frames(pkg):
    p = Pair(pkg, pipelining=2)
    src = add_sources(p)
    m = rotation((0.4, 0.4, 1.0), 0.6, t=(70.0, -30.0, 20.0))

    def frame(c, s, seed):
        prm = pkg.default_params(num_rays=8192, depth=8, seed=seed, flags=pkg._capi.FLAG_DETERMINISTIC)
        c.compute_energy_response_async(s, prm)
        c.reconstruct_impulse_response_async(s, prm)

    def publish(c, s):
        c.synchronize()
        return c.impulse_response(s, 0)

    for c, s in zip((p.a, p.b), src):
        frame(c, s, 51)                                          # held back: traced through the rest pose
    p.transform([900, 20], [m, m])                               # finishes the held frame first
    first = [publish(c, s) for c, s in zip((p.a, p.b), src)]
    for c, s in zip((p.a, p.b), src):
        frame(c, s, 51)
    second = [publish(c, s) for c, s in zip((p.a, p.b), src)]
    assert first[0].tobytes() == first[1].tobytes() and second[0].tobytes() == second[1].tobytes()
    assert first[0].any() and second[0].any() and first[0].tobytes() != second[0].tobytes()
    # and without a wait between the transform and the next frame
    for c, s in zip((p.a, p.b), src):
        frame(c, s, 52)
    p.transform([900], [IDENTITY])
    for c, s in zip((p.a, p.b), src):
        frame(c, s, 53)
    third = [publish(c, s) for c, s in zip((p.a, p.b), src)]
    assert third[0].tobytes() == third[1].tobytes()
    compare_refitted(p, "after the stream")
    p.close()


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------
def raw_call(ctx, ids, mats, count=None):
    ids = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    mats = None if mats is None else np.ascontiguousarray(mats, np.float32).reshape(-1)
    n = (0 if ids is None else ids.shape[0]) if count is None else count
    return ctx.lib.fs_scene_set_object_transforms(ctx.h, None if ids is None else ids.ctypes.data,
                                                  None if mats is None else mats.ctypes.data, n)


def whole(ctx):
    s = tc.snapshot(ctx)
    return s.header, {k: getattr(s, k).tobytes() for k in ARRAYS}


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    INVALID, NOT_COMMITTED = pkg._capi.ERR_INVALID_ARGUMENT, pkg._capi.ERR_NOT_COMMITTED
    tri, mat, obj = make_scene()
    ctx = pkg.Context(num_bands=1)
    assert raw_call(ctx, [20], IDENTITY) == NOT_COMMITTED                      # nothing registered at all
    ctx.check(ctx.lib.fs_scene_set_triangles(ctx.h, tri.ctypes.data, mat.ctypes.data, T))
    assert raw_call(ctx, [20], IDENTITY) == NOT_COMMITTED
    ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj)
    ctx.set_object_transforms([20, 11], [rotation((1, 1, 1), 0.4, t=(9.0, 8.0, 7.0)), rotation((0, 1, 0), 0.1)])
    for refit_first in (True, False):                                          # with and without a refit pending
        if refit_first:
            ctx.refit()
        else:
            ctx.set_object_transform(12, rotation((0, 0, 1), 0.3))
        before = whole(ctx)
        assert before[0]["refit_pending"] == (0 if refit_first else 1)
        nan, inf = IDENTITY.copy(), IDENTITY.copy()
        nan[1, 2] = np.nan; inf[2, 3] = np.inf
        steep, away = IDENTITY.copy(), IDENTITY.copy()
        steep[0, 1] = 1e36                                                      # 1e36 * ~2 000 leaves fp32
        away[2, 3] = -3.3e38
        cases = [("ids NULL", None, [IDENTITY], 1), ("matrices NULL", [20], None, 1), ("count 0", [20], [IDENTITY], 0),
                 ("count -1", [20], [IDENTITY], -1), ("NaN entry", [13, 20], [IDENTITY, nan], None),
                 ("infinite entry", [20], [inf], None), ("an id twice", [20, 13, 20], [IDENTITY] * 3, None),
                 ("an id without triangles", [12, 21], [IDENTITY] * 2, None),
                 ("a coordinate could leave fp32 (matrix)", [11, 900], [IDENTITY, steep], None),
                 ("a coordinate could leave fp32 (translation)", [7], [away], None)]
        for what, ids, mats, count in cases:
            assert raw_call(ctx, ids, mats, count) == INVALID, what
            after = whole(ctx)
            assert after[0] == before[0], what
            assert all(after[1][k] == before[1][k] for k in ARRAYS), what
    ctx.set_object_transform(20, IDENTITY)                                     # and the context still works
    ctx.close()
    plain = pkg.Context(num_bands=1)                                           # "every triangle its own actor" has no ids to name
    plain.set_scene(tri, mat, ABSORPTION)
    before = whole(plain)
    assert raw_call(plain, [0], [IDENTITY]) == INVALID
    after = whole(plain)
    assert after[0] == before[0] and after[1] == before[1]
    plain.close()


# ---- 8: CPU ---------------------------------------------------------------------------------------------------------------------
def test_null_arguments_without_a_device(pkg):
    lib = pkg._capi.load()
    assert lib.fs_scene_set_object_transforms(None, None, None, 0) == pkg._capi.ERR_INVALID_ARGUMENT
    ids = np.array([1], np.uint32)
    assert lib.fs_scene_set_object_transforms(None, ids.ctypes.data, IDENTITY.ctypes.data, 1) == pkg._capi.ERR_INVALID_ARGUMENT


def _error_in_ulps_of_the_largest_term(m, v):
    """|xf(m, v) - float64 evaluation| in units of ulp32(largest of the three products and the translation), per coordinate"""
    got = xf(m, v).astype(np.float64)
    m64, v64 = m.astype(np.float64), v.astype(np.float64)
    want = v64 @ m64[:, :3].T + m64[:, 3]
    terms = np.abs(np.concatenate([v64[:, None, :] * m64[None, :, :3], np.broadcast_to(m64[None, :, 3:], (v.shape[0], 3, 1))], axis=2))
    ulp = np.spacing(terms.max(axis=2).astype(np.float32)).astype(np.float64)
    return np.abs(got - want) / ulp, want


def test_restatement_against_float64():
    """xf() — what context B is fed — against a float64 evaluation of m applied to the vertex, on 10 000 random vertices, in
    ulps of the largest term L (the three products and the translation).

    To 1 ulp for a signed axis permutation with a translation (x' = -z + tx, y' = x + ty, z' = -y + tz): the products are
    exact, the sums with the zero products are exact, and the one rounded sum is at most 2 L, so its half ulp is at most
    1 ulp of L.  The matrix is not symmetric: read transposed it is off by whole units, which is what this pins.

    For a general matrix 1 ulp of L cannot be promised by ANY evaluation in fp32 with six rounded operations: three
    products of at most L (half an ulp of L each), sums of at most 2 L, 3 L and 4 L (half an ulp each: 1, 2 and 2 ulps
    of L) — 6.5 ulps of L is the bound that follows from the format, and the oblique, mirrored matrix of the GPU tests is
    held to that (it reaches 3.2)."""
    rng = np.random.default_rng(3)
    v = rng.uniform(-2000.0, 2000.0, (10000, 3)).astype(np.float32)
    perm = np.array([[0, 0, -1, 130.0], [1, 0, 0, -75.5], [0, -1, 0, 21.25]], np.float32)
    general = rotation((1.0, 2.0, -0.5), 0.77, t=(130.0, -75.5, 21.25), scale=(-1.5, 0.75, 2.0))
    for m, bound in ((perm, 1.0), (general, 6.5)):
        err, want = _error_in_ulps_of_the_largest_term(m, v)
        print("largest error: %.3f ulp of the largest term (bound %.1f)" % (err.max(), bound))
        assert err.max() <= bound, err.max()
        mt = m.copy(); mt[:, :3] = m[:, :3].T
        assert np.abs(xf(mt, v).astype(np.float64) - want).max() > 100.0
