"""FS_FLAG_ROOM_PARAMETERS: per-band room parameters published with each impulse response (fs_get_room_parameters).

The restatement below is written from the definitions (include/frequensee.h fs_room_parameters, DESIGN.md section 8 "Room
parameters"), in float64, and rounded to float32 once at the end.  The CPU part pins it to the closed forms of a geometric
decay and to the edge cases; the GPU part checks every route that publishes records against it.

Tolerance (derived, not measured): both sides compute in double; sums of <= 1e4 non-negative terms, one log and a centred
fit differ between them only by summation order (about 1e-12 relative), so after the single rounding to float the two
results are equal or one ulp apart: assert_array_max_ulp(gpu, ref, 2) per field, NaN matching NaN and +inf matching +inf.
That holds only where no input sits on a threshold (a fit point within 1e-9 dB of -5, -10, -25 or -35 dB, a bin within
1e-12 relative of max / 100, a bin time within 1e-12 s of 50 or 80 ms): the restatement flags such inputs and every test
asserts that its inputs have none.
"""
import ctypes as C
import threading

import numpy as np
import pytest

ROOM = 1024        # FS_FLAG_ROOM_PARAMETERS
FLUSH = 2          # FS_FLAG_FLUSH_BEFORE_RECONSTRUCT
DET = 8            # FS_FLAG_DETERMINISTIC
FIELDS = ("energy", "onset", "edt", "t20", "t30", "c50", "c80", "d50", "ts")
RANGES = ((-10.0, 0.0), (-25.0, -5.0), (-35.0, -5.0))   # edt, t20, t30
DB_EDGES = (-5.0, -10.0, -25.0, -35.0)
T_EDGES = (0.050, 0.080)
DT1 = float(np.float32(0.001))   # a context's default bin duration: (double) 0.001f

# id -> (sample_rate, simulated_duration, bin_duration): tests/test_config_shapes.py's shapes
SHAPES = {
    "default": (48000, 1.0, 0.001),
    "short_250ms": (48000, 0.25, 0.001),
    "sr22050_bin2ms": (22050, 1.0, 0.002),
    "masks_32": (48000, 2.7, 0.001),
    "one_bin": (48000, 0.5, 0.5),
}


# ---- the float64 restatement ------------------------------------------------------------------------------------------------
def room_parameters_f64(E, dt, db_margin=1e-9, rel_margin=1e-12, t_margin=1e-12):
    """(values [9] float64, borderline) for one band E[N] (any float dtype, taken literally); dt = (double) bin_duration"""
    E = np.asarray(E, dtype=np.float64)
    N = E.shape[0]
    nan = np.nan
    energy = float(E.sum())
    if not np.all(np.isfinite(E)) or np.any(E < 0) or not np.any(E > 0):
        return np.array([energy] + [nan] * 8), False
    pk = float(E.max())
    thr = pk / 100.0
    k0 = int(np.nonzero(E >= thr)[0][0])
    border = bool(np.any(np.abs(E - thr) <= rel_margin * thr))
    e = E[k0:]
    t = np.arange(N - k0, dtype=np.float64) * dt
    S = np.cumsum(e[::-1])[::-1]
    with np.errstate(divide="ignore"):
        L = np.where(S > 0, 10.0 * np.log10(S / S[0]), -np.inf)
    for edge in DB_EDGES:
        border = border or bool(np.any(np.abs(L - edge) <= db_margin))
    for edge in T_EDGES:
        border = border or bool(np.any(np.abs(t - edge) <= t_margin))
    decay = []
    for lo, hi in RANGES:
        sel = (L >= lo) & (L <= hi)
        if sel.sum() < 2 or not np.any(L < lo):
            decay.append(nan)
            continue
        ts_, ls_ = t[sel], L[sel]
        a, b = ts_ - ts_.mean(), ls_ - ls_.mean()
        m = float((a * b).sum() / (a * a).sum())
        decay.append(-60.0 / m if m < 0 else nan)
    early = {tau: float(e[t < tau].sum()) for tau in T_EDGES}
    late = {tau: float(e[t >= tau].sum()) for tau in T_EDGES}

    def clarity(tau):
        return 10.0 * np.log10(early[tau] / late[tau]) if late[tau] > 0 else np.inf

    total = float(e.sum())
    vals = [energy, k0 * dt] + decay + [clarity(0.050), clarity(0.080), early[0.050] / (early[0.050] + late[0.050]),
                                        float((t * e).sum()) / total]
    return np.array(vals, dtype=np.float64), border


def restate(E, dt, **margins):
    """[B][N] -> (float32 [B][9], borderline per band)"""
    E = np.atleast_2d(E)
    out, border = [], []
    for row in E:
        v, b = room_parameters_f64(row, dt, **margins)
        out.append(v.astype(np.float32))
        border.append(b)
    return np.array(out, dtype=np.float32), border


def as_matrix(rec):
    """structured array of fs_room_parameters -> float32 [B][9]"""
    return np.stack([np.asarray(rec[f], dtype=np.float32) for f in FIELDS], axis=-1)


def assert_records(got, ref, what=""):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for i, f in enumerate(FIELDS):
        g, r = got[..., i].ravel(), ref[..., i].ravel()
        print(f"{what} {f}: gpu {g.tolist()} ref {r.tolist()}")
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, f, g, r)
        assert np.array_equal(np.isposinf(g), np.isposinf(r)) and np.array_equal(np.isneginf(g), np.isneginf(r)), (what, f, g, r)
        fin = np.isfinite(r)
        if fin.any():
            np.testing.assert_array_max_ulp(g[fin], r[fin], 2)


# ---- closed forms of a geometric decay ----------------------------------------------------------------------------------------
def geometric(N, d, r):
    """E[k] = r^(k - d) from bin d on, 0 before (float64)"""
    E = np.zeros(N)
    k = np.arange(d, N)
    E[d:] = r ** (k - d)
    return E


def closed_form(N, d, r, dt):
    """every field of geometric(N, d, r) from the truncated Schroeder sum S[k] = r^(k-d) (1 - r^(N-k)) / (1 - r), k >= d"""
    M = N - d                                   # bins from the onset on
    j = np.arange(M, dtype=np.float64)
    t = j * dt
    energy = (1.0 - r ** M) / (1.0 - r)
    L = 10.0 * np.log10(r ** j * (1.0 - r ** (M - j)) / (1.0 - r ** M))
    L = np.where(M - j > 0, L, -np.inf)
    decay = []
    for lo, hi in RANGES:
        sel = (L >= lo) & (L <= hi)
        if sel.sum() < 2 or not np.any(L < lo):
            decay.append(np.nan)
            continue
        a, b = t[sel] - t[sel].mean(), L[sel] - L[sel].mean()
        m = (a * b).sum() / (a * a).sum()
        decay.append(-60.0 / m if m < 0 else np.nan)

    def split(tau):
        J = int(np.count_nonzero(t < tau))
        return (1.0 - r ** J) / (1.0 - r), (r ** J - r ** M) / (1.0 - r)

    (e50, l50), (e80, l80) = split(0.050), split(0.080)
    c = [10.0 * np.log10(e / l) if l > 0 else np.inf for e, l in ((e50, l50), (e80, l80))]
    sum_jr = r * (1.0 - M * r ** (M - 1) + (M - 1) * r ** M) / (1.0 - r) ** 2   # sum_{j < M} j r^j
    ts = dt * sum_jr / energy
    return np.array([energy, d * dt] + decay + c + [e50 / (e50 + l50), ts])


@pytest.mark.parametrize("dt", [0.0005, 0.001, 0.002])
@pytest.mark.parametrize("T", [0.37, 0.53, 0.71, 1.7])
@pytest.mark.parametrize("N,d", [(1, 0), (2, 0), (7, 2), (60, 0), (250, 5), (1000, 0), (1000, 17), (2750, 3)])
def test_restatement_matches_closed_forms(N, d, T, dt):
    """a geometric decay of T seconds (60 dB) per bin r = 10^(-6 dt / T): the restatement against the closed forms.  dt is the
    float32 bin duration widened to double, as a context has it (an exact 1 ms would put bin 50 on 50 ms: borderline)"""
    dt = float(np.float32(dt))
    if d >= N:
        d = N - 1
    r = 10.0 ** (-6.0 * dt / T)
    E = geometric(N, d, r)
    got, border = room_parameters_f64(E, dt)
    assert not border, (N, d, T, dt)
    want = closed_form(N, d, r, dt)
    print(N, d, T, dt, got.tolist(), want.tolist())
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-9, atol=1e-12)
    if N == 1:
        assert np.isnan(got[2:5]).all()
    # an untruncated decay returns its decay time (the window ends far below -35 dB)
    if (N - d) * dt >= 2.0 * T and N > 1:
        np.testing.assert_allclose(got[2:5], [T, T, T], rtol=1e-6)


def test_truncated_window_shortens_the_decay():
    """T = 2 s in a 1 s window: the truncated sum bends the curve down and t30 comes out near 1.76 s, not 2 (why the closed-form
    test uses the truncated sum)"""
    dt = DT1
    r = 10.0 ** (-6.0 * dt / 2.0)
    got, border = room_parameters_f64(geometric(1000, 0, r), dt)
    assert not border
    np.testing.assert_allclose(got[2:5], closed_form(1000, 0, r, dt)[2:5], rtol=1e-9)
    assert 1.7 < got[4] < 1.8


# ---- edge cases ---------------------------------------------------------------------------------------------------------------
def test_empty_band():
    v, border = room_parameters_f64(np.zeros(1000, np.float32), DT1)
    assert v[0] == 0.0 and np.isnan(v[1:]).all() and not border


def test_negative_bin():
    E = geometric(1000, 0, 0.99).astype(np.float32)
    E[500] = -1e-6
    v, _ = room_parameters_f64(E, DT1)
    assert v[0] == pytest.approx(float(E.astype(np.float64).sum())) and np.isnan(v[1:]).all()
    for bad in (np.nan, np.inf):
        E2 = E.copy()
        E2[3] = bad
        v, _ = room_parameters_f64(E2, DT1)
        assert np.isnan(v[1:]).all()


def test_single_nonzero_bin():
    """one bin: no decay (a single fit point), all of it early (c50 = c80 = +inf), d50 = 1, ts = 0"""
    E = np.zeros(1000, np.float32)
    E[40] = 0.25
    v, border = room_parameters_f64(E, DT1)
    assert not border
    assert v[0] == 0.25 and v[1] == pytest.approx(0.040)
    assert np.isnan(v[2:5]).all()
    assert np.isposinf(v[5]) and np.isposinf(v[6]) and v[7] == 1.0 and v[8] == 0.0


def test_decay_cut_off_before_minus_35_db():
    """the histogram ends before the decay leaves [-35, -5] dB: t30 is NaN, t20 and edt are not"""
    dt, T = DT1, 0.71
    r = 10.0 ** (-6.0 * dt / T)
    # the last bin's level L[N-1] = 10 log10(r^(N-1) (1 - r) / (1 - r^N)): take the longest N that stays above -35 dB
    N = max(n for n in range(2, 2000) if 10.0 * np.log10(r ** (n - 1) * (1.0 - r) / (1.0 - r ** n)) > -35.0)
    v, border = room_parameters_f64(geometric(N, 0, r), dt)
    assert not border
    assert np.isnan(v[4]) and np.isfinite(v[2]) and np.isfinite(v[3])
    np.testing.assert_allclose(v, closed_form(N, 0, r, dt), rtol=1e-9, equal_nan=True)


def test_large_clamp_bin():
    """the last bin collects every later arrival and is taken literally: here it is the peak, so the onset is the first bin
    within 20 dB of IT, and it is late energy"""
    dt = DT1
    E = geometric(1000, 10, 0.98)
    E[-1] = 30.0
    v, border = room_parameters_f64(E, dt)
    assert not border
    k0 = int(np.nonzero(E >= 0.3)[0][0])
    assert k0 == 10 and v[1] == pytest.approx(k0 * dt)   # (E[10] = 1 >= 30 / 100)
    assert v[0] == pytest.approx(E.sum())
    tail = E[k0:]
    t = np.arange(tail.size) * dt
    assert v[7] == pytest.approx(tail[t < 0.05].sum() / tail.sum(), rel=1e-12)
    assert v[8] == pytest.approx((t * tail).sum() / tail.sum(), rel=1e-12)
    assert v[8] > 0.3   # the clamp bin (30 of 80 units, at 0.99 s) pulls the centre time towards the end of the window


def test_late_sum_zero():
    """everything within 50 ms of the onset: c50 = c80 = +inf, d50 = 1"""
    E = geometric(1000, 3, 0.5)
    E[40:] = 0.0
    v, border = room_parameters_f64(E, DT1)
    assert not border
    assert np.isposinf(v[5]) and np.isposinf(v[6]) and v[7] == 1.0


def test_borderline_inputs_are_flagged():
    """the flag the tests assert against: an exact threshold is caught (T = 0.3 s at 1 ms bins puts bin 25 on -5 dB)"""
    dt = 0.001
    r = 10.0 ** (-6.0 * dt / 0.3)
    assert room_parameters_f64(geometric(1000, 0, r), dt)[1]
    E = np.array([1.0, 0.01, 0.5])   # a bin exactly at max / 100 ...
    assert room_parameters_f64(E, dt)[1]
    E = np.zeros(100)
    E[0], E[50] = 1.0, 0.5           # ... a bin time exactly at 50 ms
    assert room_parameters_f64(E, dt)[1]


# ---- the export ---------------------------------------------------------------------------------------------------------------
def test_room_parameters_export(pkg):
    """fs_get_room_parameters is exported and listed; its ctypes record is 36 bytes; a null context is refused"""
    import os
    lib = pkg._capi.load()
    assert hasattr(lib, "fs_get_room_parameters")
    assert "fs_get_room_parameters" in pkg._capi.EXPORTS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frequensee.h")).read()
    head = hdr[:hdr.index("#ifndef FREQUENSEE_H")]
    assert "fs_get_room_parameters" in head[head.index("EXTENDED:"):]
    assert "#define FS_FLAG_ROOM_PARAMETERS 1024u" in hdr
    assert pkg._capi.FLAG_ROOM_PARAMETERS == ROOM
    assert C.sizeof(pkg._capi.RoomParameters) == 36
    assert [k for k, _ in pkg._capi.RoomParameters._fields_] == list(FIELDS)
    rec = (pkg._capi.RoomParameters * 8)()
    seq = C.c_uint64(5)
    assert lib.fs_get_room_parameters(None, 0, rec, 1, C.byref(seq)) == pkg._capi.ERR_INVALID_ARGUMENT
    assert seq.value == 5
    import torch
    if not torch.cuda.is_available():   # (no context can be created without a device: the reader's other checks are GPU tests)
        h = C.c_void_p()
        cfg = pkg.default_config()
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == pkg._capi.ERR_NO_DEVICE
        if h:
            lib.fs_context_destroy(h)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def new_ctx(pkg, shape="default", B=1, **kw):
    sr, dur, bd = SHAPES[shape]
    return pkg.Context(num_bands=B, sample_rate=sr, simulated_duration=dur, bin_duration=bd, **kw)


def dt_of(ctx):
    return float(np.float32(ctx.cfg.bin_duration))   # Δ = (double) cfg.bin_duration


def check_source(ctx, src, what, energy=None):
    """the front publish's records against the restatement of the source's current histogram (fs_get_energy_buffer)"""
    E = ctx.energy_buffer(src) if energy is None else energy
    ref, border = restate(E, dt_of(ctx))
    assert not any(border), f"{what}: borderline input"
    seq, rec = ctx.room_parameters(src)
    assert seq != 0, what
    assert seq == ctx.impulse_response_sequence(src), what
    assert_records(as_matrix(rec), ref, what)
    return seq, as_matrix(rec)


def synthetic(rng, B, N, dt):
    """per band a noisy decay with its own onset and decay time; band 1 of 8 is empty, band 2 holds one bin"""
    E = np.zeros((B, N), np.float32)
    for b in range(B):
        T = rng.uniform(0.15, 1.5)
        d = int(rng.integers(0, max(1, N // 8)))
        r = 10.0 ** (-6.0 * dt / T)
        k = np.arange(d, N)
        E[b, d:] = (1e-3 * r ** (k - d) * rng.uniform(0.5, 1.5, N - d)).astype(np.float32)
    if B >= 8:
        E[1] = 0.0
        E[2] = 0.0
        E[2, min(5, N - 1)] = 0.5
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_synthetic_histograms(pkg, shape, B):
    ctx = new_ctx(pkg, shape, B)
    src = ctx.create_source()
    rng = np.random.default_rng(0x2007 + B)
    E = synthetic(rng, B, ctx.num_bins, dt_of(ctx))
    ctx.update_energy_buffer(src, E)
    ctx.reconstruct_impulse_response(src, pkg.default_params(flags=ROOM))
    got = ctx.energy_buffer(src)
    assert np.array_equal(got, E)
    check_source(ctx, src, f"{shape} B={B}")
    # a negative bin: every field but the energy is NaN
    E[0, -1] = -1.0
    ctx.update_energy_buffer(src, E)
    ctx.reconstruct_impulse_response(src, pkg.default_params(flags=ROOM))
    check_source(ctx, src, f"{shape} B={B} negative")
    ctx.close()


# The traced inputs below were checked on the CPU while choosing them: the oracle's histograms of the same frames (same path set
# as the GPU's, bins within ~4e-7 relative, so the margins widen to 1e-4 dB and 1e-5 relative at the onset threshold) — both
# scenes at 4 bands, both frame kinds, seed 0x5EED at the 8 source positions, seeds 0x5EED + i for the pipelined frames and
# 0x5EED + 17 i for the 48 frames of the reader test: 108 histograms, none borderline.  The GPU tests check the 1e-9 dB window
# on the histograms they read back.
SCENE_BANDS = 4
FRAMES = [(2000, 0), (65536, 8)]   # (rays, depth): 1 000 pairs unbounded, 32 768 pairs at depth 8
SEED = 0x5EED


def scene_ctx(pkg, scene_factory, name, **kw):
    sc = scene_factory(name, SCENE_BANDS)
    ctx = pkg.Context(num_bands=SCENE_BANDS, **kw)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    return ctx, sc


def source_positions(sc, n):
    """the scene's source, then points within 10 % of the scene's extent around it (seeded)"""
    rng = np.random.default_rng(n)
    lo, hi = sc.triangles.min(axis=(0, 1)), sc.triangles.max(axis=(0, 1))
    return [np.asarray(sc.source, np.float32)] + [(sc.source + rng.uniform(-0.1, 0.1, 3) * (hi - lo)).astype(np.float32)
                                                   for _ in range(n - 1)]


def frame_params(pkg, rays, depth, det, seed=SEED, extra=0):
    return pkg.default_params(num_rays=rays, depth=depth, seed=seed, flags=(DET if det else 0) | extra)


ROUTES = ["sync", "async", "batch", "update_sources", "profiling2", "flush", "pipelined"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("scene", ["starter_room", "old_mine"])
def test_traced_frames(pkg, scene_factory, scene, route):
    ctx, sc = scene_ctx(pkg, scene_factory, scene)
    nsrc = 8 if route in ("batch", "update_sources", "pipelined") else 1
    srcs = [ctx.create_source(p) for p in source_positions(sc, nsrc)]
    if route == "profiling2":
        ctx.set_profiling(2)
    for rays, depth in FRAMES:
        for det in (False, True):
            what = f"{scene} {route} rays={rays} depth={depth} det={det}"
            p = frame_params(pkg, rays, depth, det)
            rp = frame_params(pkg, rays, depth, det, extra=ROOM)
            if route in ("sync", "profiling2"):
                ctx.compute_energy_response(srcs[0], p, want_host=False)
                ctx.reconstruct_impulse_response(srcs[0], rp)
            elif route == "async":
                ctx.compute_energy_response_async(srcs[0], p)
                ctx.reconstruct_impulse_response_async(srcs[0], rp)
                ctx.synchronize()
            elif route == "batch":
                ctx.compute_energy_response_batch_async(srcs, p)
                ctx.reconstruct_impulse_response_batch_async(srcs, rp)
                ctx.synchronize()
            elif route == "update_sources":
                ctx.update_sources(srcs, rp)
            elif route == "flush":
                ctx.compute_energy_response(srcs[0], p, want_host=False)
                ctx.reconstruct_impulse_response(srcs[0], frame_params(pkg, rays, depth, det, extra=ROOM | FLUSH))
                seq, rec = ctx.room_parameters(srcs[0])
                m = as_matrix(rec)
                assert seq == ctx.impulse_response_sequence(srcs[0]) and seq != 0, what
                assert (m[:, 0] == 0.0).all() and np.isnan(m[:, 1:]).all(), (what, m)
                assert not ctx.energy_buffer(srcs[0]).any()
                continue
            elif route == "pipelined":
                ctx.set_pipelining(2)
                ctx.set_frames_per_launch(2)
                for i, s in enumerate(srcs):   # one frame per source, held two per launch; each reconstruct recorded with its frame
                    ctx.compute_energy_response_async(s, frame_params(pkg, rays, depth, det, seed=SEED + i))
                    ctx.reconstruct_impulse_response_async(s, rp)
                ctx.synchronize()
                ctx.set_frames_per_launch(1)
                ctx.set_pipelining(0)
            for s in srcs:
                check_source(ctx, s, what)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["starter_room", "old_mine"])
def test_nothing_else_changes(pkg, scene_factory, scene):
    """the IR's channel and band rows and the energy buffer are the same bits with and without the flag; an unflagged publish or
    fs_set_impulse_response after a flagged one carries no records; the same histogram gives the same records every time"""
    ctx, sc = scene_ctx(pkg, scene_factory, scene)
    src = ctx.create_source(sc.source)
    out = {}
    for flag in (0, ROOM, 0, ROOM):
        p = frame_params(pkg, 65536, 8, True)
        ctx.compute_energy_response(src, p, want_host=False)
        ctx.reconstruct_impulse_response(src, frame_params(pkg, 65536, 8, True, extra=flag))
        e = ctx.energy_buffer(src)
        ir = ctx.impulse_response(src)
        bands = np.stack([ctx.band_impulse_response(src, b) for b in range(SCENE_BANDS)])
        seq, rec = ctx.room_parameters(src)
        if flag:
            assert seq == ctx.impulse_response_sequence(src) and seq != 0
            assert_records(as_matrix(rec), restate(e, dt_of(ctx))[0], f"{scene} det frame")
            if ROOM in out:   # deterministic histograms repeat bit for bit, and so do their records
                assert as_matrix(rec).tobytes() == out[ROOM][3].tobytes()
        else:
            assert seq == 0   # an unflagged publish after a flagged one
        if flag in out:
            assert e.tobytes() == out[flag][0].tobytes()
        out[flag] = (e, ir, bands, as_matrix(rec) if flag else None)
        if 0 in out and ROOM in out:
            assert out[0][0].tobytes() == out[ROOM][0].tobytes()
            assert out[0][1].tobytes() == out[ROOM][1].tobytes()
            assert out[0][2].tobytes() == out[ROOM][2].tobytes()
    # fs_set_impulse_response after a flagged publish
    ctx.set_impulse_response(src, np.zeros(ctx.num_samples, np.float32))
    seq, rec = ctx.room_parameters(src)
    assert seq == 0 and np.isnan(as_matrix(rec)).all()   # (out untouched: the NaN the mirror filled it with)
    # the same histogram reconstructed twice: the same bits
    E = out[ROOM][0]
    recs = []
    for _ in range(2):
        ctx.update_energy_buffer(src, E)
        ctx.reconstruct_impulse_response(src, pkg.default_params(flags=ROOM))
        recs.append(check_source(ctx, src, "again")[1])
    assert recs[0].tobytes() == recs[1].tobytes() == out[ROOM][3].tobytes()
    ctx.close()


@pytest.mark.gpu
def test_reader_during_a_stream(pkg, scene_factory):
    """a thread polls fs_get_room_parameters while flagged deterministic frames with distinct seeds stream through
    fs_set_pipelining(2): every (sequence, records) it sees is the expected one for that publish, and sequences never decrease"""
    ctx, sc = scene_ctx(pkg, scene_factory, "starter_room")
    src = ctx.create_source(sc.source)
    nframes = 48
    seeds = [SEED + 17 * i for i in range(nframes)]
    base = ctx.impulse_response_sequence(src)
    seen, stop = [], threading.Event()
    lib, h = ctx.lib, ctx.h
    rec_t = pkg._capi.RoomParameters * SCENE_BANDS

    def poll():
        rec, seq = rec_t(), C.c_uint64()
        while not stop.is_set():
            rc = lib.fs_get_room_parameters(h, src, rec, SCENE_BANDS, C.byref(seq))
            assert rc == 0
            if seq.value:
                seen.append((seq.value, np.array([[getattr(rec[b], f) for f in FIELDS] for b in range(SCENE_BANDS)], np.float32)))

    th = threading.Thread(target=poll)
    th.start()
    try:
        ctx.set_pipelining(2)
        for s in seeds:
            ctx.compute_energy_response_async(src, frame_params(pkg, 65536, 8, True, seed=s))
            ctx.reconstruct_impulse_response_async(src, frame_params(pkg, 65536, 8, True, extra=ROOM))
        ctx.synchronize()
        ctx.set_pipelining(0)
    finally:
        stop.set()
        th.join()
    # the expected records: every seed traced again, waited for
    expected = {}
    for i, s in enumerate(seeds):
        ctx.compute_energy_response(src, frame_params(pkg, 65536, 8, True, seed=s), want_host=False)
        ctx.reconstruct_impulse_response(src, frame_params(pkg, 65536, 8, True, extra=ROOM))
        expected[base + 1 + i] = check_source(ctx, src, f"seed {s}")[1]
    assert len(seen) > 0
    print(f"{len(seen)} observations, {len(set(q for q, _ in seen))} distinct publishes")
    last = 0
    for q, r in seen:
        assert q >= last
        last = q
        assert q in expected, q
        assert r.tobytes() == expected[q].tobytes(), q
    ctx.close()
