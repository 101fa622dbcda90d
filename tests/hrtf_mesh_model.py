"""What the tests of the HRIR mesh share (test_hrtf_mesh_cpu.py, test_binaural_interp.py): the direction sets, a numpy float64
restatement of fs_hrtf_mesh_rows' rows and a numpy float32 restatement of fs_hrtf_mesh_locate (include/frequensee.h, "The mesh")."""
import numpy as np

F32 = np.float32


def fibonacci(n):
    """the spherical head's directions: a Fibonacci spiral from the zenith down"""
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1).astype(np.float32)


def lat_long(azimuths, elevations_deg, poles):
    """a grid of `azimuths` directions on every elevation, azimuth 0 first — exactly (cos el, 0, sin el) — then the two poles"""
    el = np.radians(np.asarray(elevations_deg, np.float64))
    az = 2.0 * np.pi * np.arange(azimuths) / azimuths
    pts = np.stack([np.outer(np.cos(el), np.cos(az)), np.outer(np.cos(el), np.sin(az)), np.outer(np.sin(el), np.ones_like(az))], 2).reshape(-1, 3)
    if poles:
        pts = np.concatenate([pts, [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]])
    return pts.astype(np.float32)


OCTAHEDRON = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
CUBE = (np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) / np.sqrt(3.0)).astype(np.float32)

# name -> directions: the sets the issue names.  "latlong": 72 x 35 with poles, elevation 0 among them, so (1, 0, 0) is in the set.
SETS = {
    "fib4": fibonacci(4), "fib5": fibonacci(5), "fib16": fibonacci(16), "fib258": fibonacci(258), "fib4096": fibonacci(4096),
    "octahedron": OCTAHEDRON, "cube": CUBE,
    "latlong": lat_long(72, np.arange(-85, 86, 5), True),
    "open": lat_long(24, np.arange(-40, 81, 10), False),
}

_meshes = {}


def mesh_of(pkg, name):
    """(dirs, tri, rows) of a named set, triangulated once by the library"""
    if name not in _meshes:
        dirs = SETS[name]
        tri = pkg.Context.hrtf_triangulate(dirs)
        _meshes[name] = (dirs, tri, pkg.Context.hrtf_mesh_rows(dirs, tri))
    return _meshes[name]


def rows64(dirs, tri):
    """r_0 = (p_b x p_c) / det, r_1 = (p_c x p_a) / det, r_2 = (p_a x p_b) / det, det = p_a . (p_b x p_c): float64 -> (rows, det)"""
    p = np.asarray(dirs, np.float32).astype(np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    bc, ca, ab = np.cross(b, c), np.cross(c, a), np.cross(a, b)
    det = np.einsum("ij,ij->i", a, bc)
    return np.stack([bc, ca, ab], 1) / det[:, None, None], det


def locate32(rows, d):
    """fs_hrtf_mesh_locate: (t, b [3]) in fp32, every operation rounded on its own, in the order written"""
    r = np.asarray(rows, np.float32)
    d = np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        g = (d[0] * r[:, :, 0] + d[1] * r[:, :, 1]) + d[2] * r[:, :, 2]   # [m][3]
        assert g.dtype == np.float32
        mu = g[:, 0].copy()
        mu = np.where(g[:, 1] < mu, g[:, 1], mu)
        mu = np.where(g[:, 2] < mu, g[:, 2], mu)
        taken = mu > F32(-np.inf)   # (not a number: never taken)
        t = int(np.argmax(np.where(taken, mu, F32(-np.inf)))) if taken.any() else 0   # the first of equal maxima
        c = np.where(g[t] > 0, g[t], F32(0.0)).astype(np.float32)
        s = F32(F32(c[0] + c[1]) + c[2])
        if s > 0:
            return t, (c / s).astype(np.float32)
    return t, np.array([1.0, 0.0, 0.0], np.float32)


def random_directions(rng, count):
    """directions of any length in [1e-3, 1e3]"""
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (d * 10.0 ** rng.uniform(-3.0, 3.0, (count, 1))).astype(np.float32)
