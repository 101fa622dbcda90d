"""The mesh on an HRIR set, host side (include/frequensee.h, "The mesh"): fs_hrtf_triangulate by its properties — the result passes
fs_hrtf_mesh_rows, has 2n - 4 triangles and no direction above a triangle's plane, and on sets in general position it is scipy's
hull —, fs_hrtf_mesh_rows against a float64 restatement and clause by clause, fs_hrtf_mesh_locate bit for bit against a numpy
float32 restatement with its ties, and what the rule is for: weights that are barycentric, that reproduce a set direction, and a
blend that is continuous where the nearest direction hops.  No device."""
import ctypes as C

import numpy as np
import pytest

from hrtf_mesh_model import F32, SETS, locate32, mesh_of, random_directions, rows64

NAMES = sorted(SETS)


def canon(tri):
    """triangles up to rotation of their indices"""
    return {tuple(np.roll(t, -int(np.argmin(t)))) for t in np.asarray(tri).tolist()}


# ---- fs_hrtf_triangulate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_triangulation_is_the_hull(pkg, name):
    dirs, tri, rows = mesh_of(pkg, name)
    n = dirs.shape[0]
    assert tri.shape == (2 * n - 4, 3) and tri.dtype == np.int32
    assert rows.shape == (2 * n - 4, 3, 3) and np.isfinite(rows).all()   # (mesh_of: fs_hrtf_mesh_rows accepted it)
    p = dirs.astype(np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    normal = np.cross(b - a, c - a)
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    height = normal @ p.T - np.einsum("ij,ij->i", normal, a)[:, None]   # of every direction over every triangle's plane
    assert height.max() <= 1e-9, f"a direction lies {height.max():.3e} above a triangle's plane"


@pytest.mark.parametrize("name", [k for k in NAMES if k.startswith("fib")])
def test_triangulation_equals_scipy_hull(pkg, name):
    spatial = pytest.importorskip("scipy.spatial")
    dirs, tri, _ = mesh_of(pkg, name)
    hull = spatial.ConvexHull(dirs.astype(np.float64))
    facets = hull.simplices.copy()
    flip = np.einsum("ij,ij->i", hull.equations[:, :3], np.cross(hull.points[facets[:, 1]] - hull.points[facets[:, 0]],
                                                                 hull.points[facets[:, 2]] - hull.points[facets[:, 0]])) < 0
    facets[flip] = facets[flip][:, ::-1]   # (scipy does not orient its simplices)
    assert canon(facets) == canon(tri)


def test_triangulation_is_quick(pkg):
    import time
    t0 = time.perf_counter()
    pkg.Context.hrtf_triangulate(SETS["fib4096"])
    assert time.perf_counter() - t0 < 2.0


def raw_triangulate(lib, dirs, n, cap, tri, m):
    return lib.fs_hrtf_triangulate(None if dirs is None else dirs.ctypes.data, n, None if tri is None else tri.ctypes.data, cap,
                                   None if m is None else C.byref(m))


def test_triangulate_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    fib = SETS["fib16"]
    circle = np.array([[np.cos(t), np.sin(t), 0.0] for t in 2 * np.pi * np.arange(12) / 12], np.float32)
    hemisphere = fib.copy()
    hemisphere[:, 2] = np.abs(hemisphere[:, 2])
    twice = fib.copy()
    twice[9] = twice[2]
    nan, inf = fib.copy(), fib.copy()
    nan[5, 1] = np.nan
    inf[0, 0] = np.inf
    many = np.zeros((4097, 3), np.float32)
    cases = [("n = 3", fib, 3, 64), ("n = 0", fib, 0, 64), ("n = 4097", many, 4097, 2 * 4097), ("one hemisphere", hemisphere, 16, 64),
             ("a great circle", circle, 12, 64), ("a duplicate direction", twice, 16, 64), ("nan", nan, 16, 64), ("inf", inf, 16, 64),
             ("cap one short", fib, 16, 27)]
    for what, dirs, n, room in cases:
        tri, m = np.full((max(room, 1), 3), -7, np.int32), C.c_int32(-7)
        assert raw_triangulate(lib, dirs, n, room, tri, m) == cap.ERR_INVALID_ARGUMENT, what
        assert np.all(tri == -7) and m.value == -7, f"{what}: a refused call wrote"
    tri, m = np.full((28, 3), -7, np.int32), C.c_int32(-7)
    for what, args in (("dirs", (None, 16, 28, tri, m)), ("tri", (fib, 16, 28, None, m)), ("m", (fib, 16, 28, tri, None))):
        assert raw_triangulate(lib, *args) == cap.ERR_INVALID_ARGUMENT, f"NULL {what}"
        assert np.all(tri == -7) and m.value == -7
    assert raw_triangulate(lib, fib, 16, 28, tri, m) == cap.OK and m.value == 28 and tri.min() >= 0
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.hrtf_triangulate(hemisphere)


# ---- fs_hrtf_mesh_rows ----------------------------------------------------------------------------------------------------------
def raw_rows(lib, dirs, n, tri, m, rows):
    return lib.fs_hrtf_mesh_rows(None if dirs is None else dirs.ctypes.data, n, None if tri is None else np.ascontiguousarray(tri).ctypes.data, m,
                                 None if rows is None else rows.ctypes.data)


def test_mesh_rows_refusals(pkg):
    """each clause of the validator broken in turn; nothing is written"""
    cap = pkg._capi
    lib = cap.load()
    dirs, tri, _ = mesh_of(pkg, "fib16")
    n, m = 16, 28
    out = np.full((m + 1, 3, 3), 7.0, np.float32)
    assert raw_rows(lib, dirs, n, tri, m, None) == cap.OK, "rows == NULL only validates"
    flipped = tri.copy()
    flipped[5] = flipped[5][::-1]
    inward = tri[:, ::-1].copy()   # closed and consistent, but every det is negative
    repeated = tri.copy()
    repeated[3] = repeated[4]   # (a missing triangle: its edges now miss their reverses, another's occur twice)
    out_of_range, negative, degenerate = tri.copy(), tri.copy(), tri.copy()
    out_of_range[7, 1] = n
    negative[0, 0] = -1
    degenerate[2, 2] = degenerate[2, 0]
    # an unused direction: the mesh of 15 directions, closed and outward, offered for 16 (m is then off as well) and, with
    # m == 2n - 4 kept, the mesh of 16 with direction 15 renamed to one of its neighbours
    tri15 = pkg.Context.hrtf_triangulate(dirs[:15])
    unused = tri.copy()
    unused[unused == 15] = int(tri[np.nonzero(tri == 15)[0][0]][(np.nonzero(tri == 15)[1][0] + 1) % 3])
    flat = np.concatenate([dirs[:15], dirs[:1]])   # a duplicate: some det is 0
    nan = dirs.copy()
    nan[3, 0] = np.nan
    many_dirs, many_tri = np.zeros((4097, 3), np.float32), np.zeros((2 * 4097 - 4, 3), np.int32)
    cases = [("a flipped triangle", dirs, n, flipped, m), ("every triangle flipped", dirs, n, inward, m), ("a missing triangle", dirs, n, repeated, m),
             ("m one short", dirs, n, tri[:-1], m - 1), ("m one more", dirs, n, np.concatenate([tri, tri[:1]]), m + 1),
             ("an index out of range", dirs, n, out_of_range, m), ("a negative index", dirs, n, negative, m),
             ("two equal indices", dirs, n, degenerate, m), ("an unused direction", dirs, n, unused, m),
             ("the mesh of fewer directions", dirs, n, tri15, tri15.shape[0]), ("det == 0", flat, n, tri, m), ("nan", nan, n, tri, m),
             ("n = 3", dirs, 3, tri[:2], 2), ("n = 4097", many_dirs, 4097, many_tri, many_tri.shape[0]), ("m = 0", dirs, n, tri, 0)]
    for what, d, nn, t, mm in cases:
        for dest in (out, None):
            assert raw_rows(lib, d, nn, t, mm, dest) == cap.ERR_INVALID_ARGUMENT, what
        assert np.all(out == 7.0), f"{what}: a refused call wrote"
    assert raw_rows(lib, None, n, tri, m, out) == cap.ERR_INVALID_ARGUMENT and raw_rows(lib, dirs, n, None, m, out) == cap.ERR_INVALID_ARGUMENT
    assert np.all(out == 7.0)
    assert raw_rows(lib, dirs, n, tri, m, out) == cap.OK and np.all(out[:m] != 7.0) and np.all(out[m] == 7.0)
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.hrtf_mesh_rows(dirs, flipped)


@pytest.mark.parametrize("name", NAMES)
def test_mesh_rows_against_float64(pkg, name):
    """computed in double and rounded once: within one float32 ulp of numpy's float64, and det >= 1e-6 as the validator asks"""
    dirs, tri, rows = mesh_of(pkg, name)
    want, det = rows64(dirs, tri)
    assert det.min() >= 1e-6
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(rows.astype(np.float64) - want) <= ulp), float(np.max(np.abs(rows.astype(np.float64) - want) / ulp))
    # r_i . p_j = delta_ij: what makes g the coefficients of d in the corners
    p = dirs.astype(np.float64)[tri]   # [m][3][3]
    assert np.abs(np.einsum("mic,mjc->mij", want, p) - np.eye(3)).max() <= 1e-9


# ---- fs_hrtf_mesh_locate --------------------------------------------------------------------------------------------------------
def assert_locates(pkg, rows, d, where):
    t, b = pkg.Context.hrtf_mesh_locate(rows, d)
    wt, wb = locate32(rows, d)
    assert (t, b.tobytes()) == (wt, wb.tobytes()), f"{where}: d = {d}: ({t}, {b}) != ({wt}, {wb})"
    return t, b


@pytest.mark.parametrize("name", NAMES)
def test_locate_bit_equal_to_the_restatement(pkg, name):
    dirs, tri, rows = mesh_of(pkg, name)
    rng = np.random.default_rng(len(name) + dirs.shape[0])
    for d in random_directions(rng, 48 if dirs.shape[0] > 1000 else 200):
        assert_locates(pkg, rows, d, name)
    for k in rng.integers(0, dirs.shape[0], 24):   # at a set direction many triangles tie or nearly tie
        assert_locates(pkg, rows, dirs[k] * F32(rng.choice([0.25, 1.0, 3.0])), f"{name}, direction {k}")


TIE_PLANTS = {1: [0], 63: [40, 10], 64: [63, 3], 65: [64, 1], 8188: [8187, 70 + 64 * 5 + 3, 70, 4096]}


@pytest.mark.parametrize("m", sorted(TIE_PLANTS))
def test_locate_exact_ties_resolve_to_the_lowest_index(pkg, m):
    """synthetic rows: one row triple, whose mu beats every other triangle's, planted at indices that fall in different strides of
    64 and at different places within them — the lowest wins, whichever order a strided search meets them in"""
    rng = np.random.default_rng(m)
    rows = rng.uniform(-1.0, 1.0, (m, 3, 3)).astype(np.float32)   # |g| <= 3 for d = (1, 1, 1)
    plant = np.array([[4.0, 0.5, 0.25], [0.5, 5.0, 0.25], [0.25, 0.5, 6.0]], np.float32)   # g = (4.75, 5.75, 6.75)
    for j in TIE_PLANTS[m]:
        rows[j] = plant
    d = np.ones(3, np.float32)
    t, b = assert_locates(pkg, rows, d, f"m = {m}")
    assert t == min(TIE_PLANTS[m])
    assert b.tobytes() == (np.array([4.75, 5.75, 6.75], np.float32) / F32(17.25)).tobytes()
    for extra in random_directions(rng, 16):
        assert_locates(pkg, rows, extra, f"m = {m}")


def test_locate_fallback_and_refusals(pkg):
    """s == 0: every g of the chosen triangle is <= 0 and b = (1, 0, 0); a NULL or m < 1 is refused and writes nothing"""
    cap = pkg._capi
    lib = cap.load()
    rows = -np.tile(np.eye(3, dtype=np.float32), (5, 1, 1))
    rows[3] *= F32(0.5)   # mu = -0.5 there, -1 elsewhere
    t, b = assert_locates(pkg, rows, np.ones(3, np.float32), "all negative")
    assert t == 3 and b.tolist() == [1.0, 0.0, 0.0]
    t, b = assert_locates(pkg, np.zeros((4, 3, 3), np.float32), np.ones(3, np.float32), "all zero")
    assert t == 0 and b.tolist() == [1.0, 0.0, 0.0]
    d = np.ones(3, np.float32)
    tt, bb = C.c_int32(-7), np.full(3, 7.0, np.float32)
    for args in ((None, 5, d.ctypes.data, C.byref(tt), bb.ctypes.data), (rows.ctypes.data, 5, None, C.byref(tt), bb.ctypes.data),
                 (rows.ctypes.data, 5, d.ctypes.data, None, bb.ctypes.data), (rows.ctypes.data, 5, d.ctypes.data, C.byref(tt), None),
                 (rows.ctypes.data, 0, d.ctypes.data, C.byref(tt), bb.ctypes.data), (rows.ctypes.data, -1, d.ctypes.data, C.byref(tt), bb.ctypes.data)):
        assert lib.fs_hrtf_mesh_locate(*args) == cap.ERR_INVALID_ARGUMENT
        assert tt.value == -7 and np.all(bb == 7.0)


# ---- what the rule is for -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_weights_are_barycentric(pkg, name):
    """b_i >= 0 and the sum within 2 ulp of 1; at a set direction the weight of that corner is at least 1 - 4e-6 (the rows are
    rounded to float and so is the dot product: an error of a few 2^-24 times |r| |p| / 1, at most about 1.7e-6 at n = 4096)"""
    dirs, tri, rows = mesh_of(pkg, name)
    rng = np.random.default_rng(7 + dirs.shape[0])
    for d in random_directions(rng, 48 if dirs.shape[0] > 1000 else 200):
        t, b = pkg.Context.hrtf_mesh_locate(rows, d)
        assert 0 <= t < tri.shape[0] and np.all(b >= 0.0)
        assert abs(float(b.astype(np.float64).sum()) - 1.0) <= 2.0 * 2.0 ** -23, (d, b)
    worst = 0.0
    picks = range(dirs.shape[0]) if dirs.shape[0] <= 400 else rng.integers(0, dirs.shape[0], 64)
    for k in picks:
        t, b = pkg.Context.hrtf_mesh_locate(rows, dirs[k])
        corner = np.nonzero(tri[t] == k)[0]
        assert corner.size == 1, f"direction {k} is located in triangle {tri[t]}, of which it is no corner"
        worst = max(worst, 1.0 - float(b[corner[0]]))
    print(f"{name}: at a set direction the corner's weight is at least 1 - {worst:.2e}")
    assert worst <= 4e-6


@pytest.mark.parametrize("name", ["fib258", "latlong"])
def test_the_blend_is_continuous_where_the_nearest_direction_hops(pkg, name):
    """a smooth per-direction table — 16 "taps" linear in the direction — blended along a tilted great circle: with twice the steps
    the largest step-to-step change halves (a ratio of at most 0.55), while the nearest direction's largest step does not shrink at
    all: the hop from one measured direction to the next, which the mesh removes"""
    dirs, tri, rows = mesh_of(pkg, name)
    rng = np.random.default_rng(11)
    table = dirs.astype(np.float64) @ rng.uniform(-1.0, 1.0, (3, 16))
    u, v = np.array([1.0, 0.0, 0.0]), np.array([0.0, np.cos(0.4), np.sin(0.4)])

    def largest_steps(steps):
        theta = 2.0 * np.pi * np.arange(steps + 1) / steps
        blended, nearest = np.zeros((steps + 1, 16)), np.zeros((steps + 1, 16))
        for k, th in enumerate(theta):
            d = (np.cos(th) * u + np.sin(th) * v).astype(np.float32)
            t, b = pkg.Context.hrtf_mesh_locate(rows, d)
            blended[k] = b.astype(np.float64) @ table[tri[t]]
            nearest[k] = table[int(np.argmax((d[0] * dirs[:, 0] + d[1] * dirs[:, 1]) + d[2] * dirs[:, 2]))]
        return np.abs(np.diff(blended, axis=0)).max(), np.abs(np.diff(nearest, axis=0)).max()

    coarse, fine = largest_steps(2000), largest_steps(4000)
    print(f"{name}: blended {coarse[0]:.3e} -> {fine[0]:.3e} (ratio {fine[0] / coarse[0]:.3f}), nearest {coarse[1]:.3e} -> {fine[1]:.3e}")
    assert fine[0] <= 0.55 * coarse[0]
    assert fine[1] >= coarse[1] > 10.0 * coarse[0]
