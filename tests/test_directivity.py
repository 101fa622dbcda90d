"""Source directivity (fs_source_set_orientation / fs_source_set_directivity, include/frequensee.h): every deposit of a
connected path gets the factor D_b(theta) of the direction w_e the path left the source in.

The yardstick is a per-pair restatement built from the oracle's exported pieces (generate_path, connect, evaluate_path,
mis_weight, add_energy_at_delay) with the emitting ray recovered from fso_philox4x32_10 + fso_sample_sphere under
fso_draw's counter layout.  The CPU test pins it against Scene.compute_energy without a table; the GPU tests hold the
kernels to it, to a closed form, and to the omnidirectional kernels bit for bit wherever the weight is 1.
"""
import ctypes as C

import numpy as np
import pytest

DET = 8                    # FS_FLAG_DETERMINISTIC (the oracle's bit 8 is its brute-force switch: never passed to it)
ALLC, MIS, LOBES, ACC, DPOS = 16, 32, 64, 128, 256
KPI = np.float32(3.1415926535897932)
TIGHT_TOL = 2e-5           # the parity bar of tests/test_gpu_parity.py
F32 = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------
def unit_fwd(f):
    f = np.asarray(f, np.float32)
    l2 = f[0] * f[0] + f[1] * f[1] + f[2] * f[2]
    return f / np.sqrt(F32(l2))


def dir_gains(table, fwd, w):
    """D_b for emission direction w (float32 arithmetic in the library's order); None = omnidirectional"""
    if table is None:
        return None
    T = np.asarray(table, np.float32)
    K = T.shape[1]
    fx, fy, fz = (F32(v) for v in fwd)
    wx, wy, wz = (F32(v) for v in w)
    cx, cy, cz = wy * fz - wz * fy, wz * fx - wx * fz, wx * fy - wy * fx
    sn = np.sqrt(F32(cx * cx + cy * cy + cz * cz))
    cs = F32(wx * fx + wy * fy + wz * fz)
    with np.errstate(invalid="ignore"):
        x = F32(np.arctan2(sn, cs) * F32(K - 1) / KPI)
    if not x >= 0:
        x = F32(0)
    k = min(int(x), K - 2)
    t = F32(x - F32(k))
    return (T[:, k] + t * (T[:, k + 1] - T[:, k])).astype(np.float32)


def seg_len(a, b, dist_divisor):
    dx, dy, dz = (F32(b.pos[i]) - F32(a.pos[i]) for i in range(3))
    return F32(np.sqrt(F32(dx * dx + dy * dy + dz * dz)) / F32(dist_divisor))


def conn_dir(a, b):
    dx, dy, dz = (F32(b.pos[i]) - F32(a.pos[i]) for i in range(3))
    l2 = F32(dx * dx + dy * dy + dz * dz)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F32(1) / np.sqrt(l2)
        return dx * inv, dy * inv, dz * inv


def emission(lib, op, pair, fwd_nodes):
    """(step, direction) of the source walk's first step with a length, or (-1, None): it never left the source"""
    for k in range(len(fwd_nodes) - 1):
        if seg_len(fwd_nodes[k], fwd_nodes[k + 1], op.dist_divisor) != 0:
            ctr = (C.c_uint32 * 4)(pair, k << 1, 0, 0x46533031)
            key = (C.c_uint32 * 2)(op.seed & 0xFFFFFFFF, op.seed >> 32)
            r = (C.c_uint32 * 4)()
            lib.fso_philox4x32_10(ctr, key, r)
            d = (C.c_float * 3)()
            lib.fso_sample_sphere(op.seed, pair, 0, k, r, d)
            return k, (F32(d[0]), F32(d[1]), F32(d[2]))
    return -1, None


def restate(oracle_mod, osc, op, src, lis, table=None, fwd=(1.0, 0.0, 0.0), pairs=None, num_bins=1000, max_nodes=600, pair_begin=0):
    """UpdateSource up to the deposit, pair by pair, with the directivity factor last; returns (e32, e64).  The pairs
    [pair_begin, pairs) are restated (pairs None: to the frame's last)"""
    lib, B = osc.lib, osc.B
    e32 = np.zeros((B, num_bins), np.float32)
    e64 = np.zeros((B, num_bins), np.float64)
    f = unit_fwd(fwd)
    norm = F32(1.0 / 1000.0) if op.flags & 1 else F32(1) / F32(op.num_pairs)
    allc = op.flags & (ALLC | MIS)
    D = op.depth
    assert D > 0 or not allc
    for i in range(pair_begin, op.num_pairs if pairs is None else pairs):
        fw = osc.generate_path(op, i, 0, src, max_nodes)
        bw = osc.generate_path(op, i, 1, lis, max_nodes)
        assert len(fw) < max_nodes and len(bw) < max_nodes
        ke, we = emission(lib, op, i, fw) if table is not None else (-1, None)
        combos = [(fi, bj) for fi in range(len(fw)) for bj in range(len(bw))] if allc else [(len(fw) - 1, len(bw) - 1)]
        for fi, bj in combos:
            if not osc.connect(op, fw[fi], bw[bj]):
                continue
            nodes = [oracle_mod.Node.from_buffer_copy(n) for n in fw[:fi + 1]] + \
                    [oracle_mod.Node.from_buffer_copy(bw[bj - j]) for j in range(bj + 1)]
            w = None
            if allc:
                for v in (fi, fi + 1):
                    if nodes[v].material != oracle_mod.NO_MATERIAL:
                        nodes[v].material &= 0xFFFF
                t = fi + bj
                lo, hi = max(t - D, 0), min(t, D)
                w = F32(1) / F32(hi - lo + 1)
                if op.flags & MIS:
                    w = F32(oracle_mod.mis_weight(nodes, fi, D))
            gains, delay = osc.evaluate_path(op, nodes)
            left = ke >= 0 and (ke < fi if allc else True)
            db = dir_gains(table, f, we if left else conn_dir(fw[fi], bw[bj]))
            for b in range(B):
                e = F32(gains[b] * norm)
                if w is not None:
                    e = F32(e * w)
                if db is not None:
                    e = F32(e * db[b])
                bin_ = oracle_mod.add_energy_at_delay(e32[b], delay, float(e))
                e64[b, bin_] += float(e)
    return e32, e64


def cardioid(bands, K=37, floor=0.02):
    """a cardioid whose power rises with the band: narrower at high frequencies"""
    th = np.arange(K) * np.pi / (K - 1)
    return np.stack([(0.5 * (1.0 + np.cos(th))) ** (1 + 1.5 * b) + floor for b in range(bands)]).astype(np.float32)


def cone(bands, K=181):
    """full gain inside 50 degrees, a ramp to the outer gain by 80 degrees, outer gain falling with the band"""
    deg = np.arange(K) * 180.0 / (K - 1)
    ramp = np.clip((deg - 50.0) / 30.0, 0.0, 1.0)
    return np.stack([1.0 + ramp * ((0.3 / (1 + b)) - 1.0) for b in range(bands)]).astype(np.float32)


OBLIQUE = (0.3, -0.8, 0.52)


def lobe_scene(oracle_mod, pkg, sc, lobes):
    tau, sigma = pkg.scenes.material_lobes(sc) if lobes else (None, None)
    return oracle_mod.Scene(sc.triangles, sc.material_ids, sc.absorption, transmission=tau, scattering=sigma), tau, sigma


# ---- CPU: the yardstick before it judges the kernels -------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ALLC, MIS, LOBES], ids=["default", "all_connections", "mis_balance", "material_lobes"])
@pytest.mark.parametrize("name,bands,rays,pairs", [("shoebox", 1, 2048, None), ("starter_room", 4, 16384, 300)])
def test_restatement_reproduces_compute_energy(pkg, oracle_mod, scene_factory, name, bands, rays, pairs, flags):
    """without a table the per-pair restatement is Scene.compute_energy bit for bit (fp32 buffer, same order of deposits)"""
    sc = scene_factory(name, bands)
    osc, _, _ = lobe_scene(oracle_mod, pkg, sc, flags & LOBES)
    op = oracle_mod.default_params(num_pairs=rays // 2, depth=6, seed=0x5EED, flags=flags)
    n = op.num_pairs if pairs is None else pairs
    e32, _, cnt = osc.compute_energy(op, sc.source, sc.listener, 0, n)
    r32, _ = restate(oracle_mod, osc, op, sc.source, sc.listener, pairs=n)
    assert cnt.connected > 0
    assert np.array_equal(r32.view(np.uint32), e32.view(np.uint32))
    # an all-ones table changes no bit either; a real one changes the result
    ones, _ = restate(oracle_mod, osc, op, sc.source, sc.listener, table=np.ones((bands, 5), np.float32), fwd=OBLIQUE, pairs=n)
    assert np.array_equal(ones.view(np.uint32), e32.view(np.uint32))
    card, _ = restate(oracle_mod, osc, op, sc.source, sc.listener, table=cardioid(bands), fwd=OBLIQUE, pairs=min(n, 200))
    assert not np.array_equal(card, restate(oracle_mod, osc, op, sc.source, sc.listener, pairs=min(n, 200))[0])


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((a - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-300))


def make_ctx(pkg, sc, tau=None, sigma=None, **kw):
    ctx = pkg.Context(num_bands=sc.num_bands, **kw)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption, transmission=tau, scattering=sigma)
    ctx.set_listener(sc.listener)
    return ctx, ctx.create_source(sc.source)


def far_triangle_scene(pkg, bands):
    """one small triangle 1 km away; source and listener 8 m apart on the x axis"""
    sc = pkg.scenes.shoebox(bands)
    sc.triangles = np.array([[[-100000.0, -50.0, -50.0], [-100000.0, 50.0, -50.0], [-100000.0, 0.0, 50.0]]], np.float32)
    sc.material_ids = np.zeros(1, np.uint16)
    sc.absorption = np.full((1, bands), 0.5, np.float32)
    sc.source = np.array([0.0, 0.0, 0.0], np.float32)
    sc.listener = np.array([800.0, 0.0, 0.0], np.float32)
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, DPOS], ids=["float_positions", "double_positions"])
def test_closed_form_direct_path(pkg, flags):
    """the direct path leaves along (L - S) / |L - S|: the direct bin's energy over the omnidirectional one is D_b(theta)
    for forwards at 0, 37, 90, 143.5 and 180 degrees from it, per band"""
    sc = far_triangle_scene(pkg, 4)
    K = 19
    th = np.arange(K) * np.pi / (K - 1)
    table = np.stack([1.0 + 0.5 * b + (0.8 - 0.15 * b) * np.cos(th * (1 + b)) for b in range(4)]).astype(np.float32)
    ctx, s = make_ctx(pkg, sc)
    p = pkg.default_params(num_rays=8192, depth=8, seed=0x5EED, flags=flags)
    omni = ctx.compute_energy_response(s, p).copy()
    direct = int(np.argmax(omni[0]))
    assert omni[0, direct] > 0.99 * omni[0].sum()       # nearly every walk stays where it starts
    ctx.set_source_directivity(s, table)
    for deg in (0.0, 37.0, 90.0, 143.5, 180.0):
        a = np.deg2rad(deg)
        ctx.set_source_orientation(s, (np.cos(a), np.sin(a), 0.0))
        e = ctx.compute_energy_response(s, p)
        want = np.array([np.interp(a * (K - 1) / np.pi, np.arange(K), table[b]) for b in range(4)])
        got = e[:, direct].astype(np.float64) / omni[:, direct]
        assert np.allclose(got, want, rtol=1e-5, atol=0), (deg, got, want)
    ctx.close()


PARITY = [
    # id, scene, bands, flags, depth, table
    ("cfg1_cardioid", "shoebox", 1, 0, 8, "cardioid"),
    ("cfg1_cone", "shoebox", 1, 0, 8, "cone"),
    ("cfg2_cardioid", "starter_room", 4, 0, 8, "cardioid"),
    ("cfg2_cone", "starter_room", 4, 0, 8, "cone"),
    ("cfg1_all_connections", "shoebox", 1, ALLC, 8, "cardioid"),
    ("cfg1_mis_balance", "shoebox", 1, MIS, 8, "cone"),
    ("cfg2_material_lobes", "starter_room", 4, LOBES, 8, "cardioid"),
    ("cfg1_depth0", "shoebox", 1, 0, 0, "cone"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,name,bands,flags,depth,tab", PARITY, ids=[c[0] for c in PARITY])
def test_parity_with_restatement(pkg, oracle_mod, scene_factory, cid, name, bands, flags, depth, tab):
    """the directional kernels against the restatement: same non-zero bins, per-band relative RMS <= 2e-5"""
    sc = scene_factory(name, bands)
    osc, tau, sigma = lobe_scene(oracle_mod, pkg, sc, flags & LOBES)
    table = cardioid(bands) if tab == "cardioid" else cone(bands)
    ctx, s = make_ctx(pkg, sc, tau, sigma)
    ctx.set_source_orientation(s, OBLIQUE)
    ctx.set_source_directivity(s, table)
    rays = 16384
    e_gpu = ctx.compute_energy_response(s, pkg.default_params(num_rays=rays, depth=depth, seed=0x5EED, flags=flags))
    e_omni = ctx.compute_energy_response(ctx.create_source(sc.source), pkg.default_params(num_rays=rays, depth=depth, seed=0x5EED, flags=flags))
    ctx.close()
    op = oracle_mod.default_params(num_pairs=rays // 2, depth=depth, seed=0x5EED, flags=flags)
    e32, e64 = restate(oracle_mod, osc, op, sc.source, sc.listener, table=table, fwd=OBLIQUE)
    assert np.array_equal(e_gpu != 0, e32 != 0)
    for b in range(bands):
        assert rel_rms(e_gpu[b], e64[b]) <= TIGHT_TOL, (b, rel_rms(e_gpu[b], e64[b]))
    assert rel_rms(e_gpu, e_omni) > 1e-3          # the pattern does change the result


IDENTITY_FLAGS = [0, ALLC, MIS, LOBES, DPOS, ACC]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", IDENTITY_FLAGS, ids=["default", "all_connections", "mis_balance", "material_lobes",
                                                       "double_positions", "accumulate"])
def test_identity_where_the_weight_is_one(pkg, scene_factory, flags):
    """FS_FLAG_DETERMINISTIC: an all-ones table, an orientation without a table, a table later cleared and a destroyed and
    re-created handle all give the omnidirectional energy bit for bit (against an omnidirectional context that traces the
    same frames)"""
    sc = scene_factory("starter_room", 4)
    tau, sigma = pkg.scenes.material_lobes(sc) if flags & LOBES else (None, None)
    p = pkg.default_params(num_rays=8192, depth=6, seed=0xD1, flags=flags | DET)
    frames = 2 if flags & ACC else 1
    ref_ctx, _ = make_ctx(pkg, sc, tau, sigma)
    ctx, s = make_ctx(pkg, sc, tau, sigma)

    def run(c, src):
        for _ in range(frames):
            e = c.compute_energy_response(src, p).copy()
        return e

    def same(src):   # every variant on a new source of each context (FS_FLAG_ACCUMULATE_ENERGY: a buffer keeps what it held)
        return np.array_equal(run(ctx, src), run(ref_ctx, ref_ctx.create_source(sc.source)))

    def fresh(table=None, forward=OBLIQUE):
        x = ctx.create_source(sc.source)
        ctx.set_source_orientation(x, forward)
        ctx.set_source_directivity(x, table)
        return x

    assert same(fresh(np.ones((4, 7), np.float32)))          # an all-ones table
    assert same(fresh())                                     # orientation only
    x = fresh(cone(4))
    assert not same(x)
    ctx.set_source_directivity(x, None)                      # cleared after it traced
    if not flags & ACC:                                      # (under FS_FLAG_ACCUMULATE_ENERGY its buffer holds a directional frame)
        assert same(x)
    y = fresh(cone(4))
    ctx.set_source_directivity(y, None)                      # cleared before it traced
    assert same(y)
    ctx.destroy_source(s)
    z = fresh(cone(4))
    ctx.destroy_source(z)
    s2 = ctx.create_source(sc.source)                        # a re-created handle: omnidirectional, facing (1, 0, 0)
    assert s2 in (s, z)
    assert same(s2)
    ctx.close()
    ref_ctx.close()


def sources_of(sc, n):
    return [np.asarray(sc.source, np.float32) + np.float32(35.0 * i) * np.array([1, 0.5, 0], np.float32) for i in range(n)]


@pytest.mark.gpu
def test_routes_agree(pkg, scene_factory, monkeypatch):
    """deterministic mode: the directional frame is the same bits on every route that traces a source"""
    sc = scene_factory("starter_room", 4)
    tables = [cardioid(4), None, cone(4)]
    fwds = [OBLIQUE, (0.0, 1.0, 0.0), (-1.0, 0.2, 0.1)]
    pos = sources_of(sc, 3)
    ctx, _ = make_ctx(pkg, sc)
    src = [ctx.create_source(x) for x in pos]
    for s, t, f in zip(src, tables, fwds):
        ctx.set_source_orientation(s, f)
        ctx.set_source_directivity(s, t)
    p = pkg.default_params(num_rays=8192, depth=8, seed=0xA1, flags=DET)
    alone = [ctx.compute_energy_response(s, p).copy() for s in src]
    assert all(a.any() for a in alone)
    # _async + fs_synchronize
    ctx.compute_energy_response_async(src[0], p)
    ctx.synchronize()
    assert np.array_equal(ctx.energy_buffer(src[0]), alone[0])
    # one batched frame of three sources (one omnidirectional)
    ctx.compute_energy_response_batch_async(src, p)
    ctx.synchronize()
    for s, a in zip(src, alone):
        assert np.array_equal(ctx.energy_buffer(s), a)
    # a depth = 0 tick
    p0 = pkg.default_params(num_rays=8192, depth=0, seed=0xA2, flags=DET)
    alone0 = [ctx.compute_energy_response(s, p0).copy() for s in src]
    ctx.update_sources(src, p0)
    for s, a in zip(src, alone0):
        assert np.array_equal(ctx.energy_buffer(s), a)
    ctx.close()

    # a pipelined stream alternating omnidirectional and directional frames, the orientation changed before every call
    def stream(pipelined):
        c, _ = make_ctx(pkg, sc)
        ss = [c.create_source(x) for x in sources_of(sc, 4)]
        c.set_source_directivity(ss[1], cardioid(4))
        c.set_source_directivity(ss[3], cone(4))
        if pipelined:
            c.set_pipelining(2)
        out = []
        for it in range(3):
            for k, s in enumerate(ss):
                a = 0.7 * it + 1.3 * k
                c.set_source_orientation(s, (np.cos(a), np.sin(a), 0.3))
                c.compute_energy_response_async(s, pkg.default_params(num_rays=8192, depth=8, seed=100 + 4 * it + k, flags=DET))
            c.synchronize()
            out += [c.energy_buffer(s).copy() for s in ss]
        c.close()
        return out
    for a, b in zip(stream(True), stream(False)):
        assert np.array_equal(a, b)

    # a staged 262 144-ray depth = 0 frame (the library's default: stages and the long-walk lane) against the walk in one piece
    big = pkg.default_params(num_rays=262144, depth=0, seed=0xA3, flags=DET)
    got = []
    for mode in ("staged", "whole"):
        for k in ("FS_SYNC_WALK_STAGES", "FS_SYNC_LANE", "FS_SYNC_STAGE_FROM"):
            monkeypatch.delenv(k, raising=False)
        if mode == "whole":
            monkeypatch.setenv("FS_SYNC_WALK_STAGES", "")
            monkeypatch.setenv("FS_SYNC_LANE", "0")
        c, s = make_ctx(pkg, sc)
        c.set_source_orientation(s, OBLIQUE)
        c.set_source_directivity(s, cone(4))
        got.append(c.compute_energy_response(s, big).copy())
        if mode == "staged":
            assert c.pipeline_counters()["lane_launches"] > 0
        c.close()
    assert np.array_equal(got[0], got[1])


@pytest.mark.gpu
def test_set_calls_do_not_reach_an_enqueued_frame(pkg, scene_factory):
    """set calls between an _async call and its fs_synchronize leave that frame bit-identical"""
    sc = scene_factory("starter_room", 4)
    p = pkg.default_params(num_rays=16384, depth=8, seed=0x5A, flags=DET)
    ctx, s = make_ctx(pkg, sc)
    ctx.set_source_orientation(s, OBLIQUE)
    ctx.set_source_directivity(s, cardioid(4))
    want = ctx.compute_energy_response(s, p).copy()
    for change in ("table", "orientation", "clear"):
        ctx.set_source_orientation(s, OBLIQUE)
        ctx.set_source_directivity(s, cardioid(4))
        ctx.compute_energy_response_async(s, p)
        if change == "table":
            ctx.set_source_directivity(s, cone(4))
        elif change == "orientation":
            ctx.set_source_orientation(s, (0.0, 0.0, -1.0))
        else:
            ctx.set_source_directivity(s, None)
        ctx.synchronize()
        assert np.array_equal(ctx.energy_buffer(s), want), change
    ctx.close()


@pytest.mark.gpu
def test_bad_input_is_refused_and_changes_nothing(pkg, scene_factory):
    sc = scene_factory("starter_room", 4)
    p = pkg.default_params(num_rays=4096, depth=6, seed=0x77, flags=DET)
    ctx, s = make_ctx(pkg, sc)
    ctx.set_source_orientation(s, OBLIQUE)
    ctx.set_source_directivity(s, cardioid(4))
    want = ctx.compute_energy_response(s, p).copy()
    bad_tables = [cardioid(3), np.ones((4, 1), np.float32), np.ones((4, 182), np.float32)]
    for v in (np.nan, np.inf, -1e-3):
        t = cone(4)
        t[2, 5] = v
        bad_tables.append(t)
    for t in bad_tables:
        with pytest.raises(pkg.FrequenSeeError) as ei:
            ctx.set_source_directivity(s, t)
        assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    for f in [(0.0, 0.0, 0.0), (np.nan, 1.0, 0.0), (np.inf, 0.0, 0.0)]:
        with pytest.raises(pkg.FrequenSeeError) as ei:
            ctx.set_source_orientation(s, f)
        assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    with pytest.raises(pkg.FrequenSeeError) as ei:
        ctx.set_source_directivity(s + 17, cone(4))
    assert ei.value.code == pkg._capi.ERR_BAD_HANDLE
    with pytest.raises(pkg.FrequenSeeError) as ei:
        ctx.set_source_orientation(s + 17, OBLIQUE)
    assert ei.value.code == pkg._capi.ERR_BAD_HANDLE
    assert np.array_equal(ctx.compute_energy_response(s, p), want)
    ctx.set_source_directivity(s, np.ones((4, 181), np.float32))    # the edges of the sample range are accepted
    ctx.set_source_directivity(s, np.ones((4, 2), np.float32))
    ctx.close()
