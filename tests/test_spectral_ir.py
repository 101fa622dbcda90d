"""FS_FLAG_SPECTRAL_IR: the channel view as per-band noise carriers shaped by the band envelopes.

The carriers and the spectral channel are restated here in numpy (float64) from the definition in include/frequensee.h:
  K = next power of two >= N; bin k in [1, K/2) at k fs / K Hz belongs to band b when edge_b <= f < edge_{b+1};
  phi_k = 2 pi (splitmix64(0x5EED + k) >> 40) 2^-24; r_b[n] = sum_{k in b} cos(2 pi k n / K + phi_k), n < N;
  c_b = r_b sqrt(N / sum r_b^2); y = (1/sqrt(B)) sum_b env_b c_b, env_b = the band row."""
import ctypes as C
import threading

import numpy as np
import pytest

SEED = 0x5EED
FLAG = 512
DET = 8   # FS_FLAG_DETERMINISTIC: integer deposits, the same energy however the frame is scheduled
FRAME = 1024


def splitmix64(x):
    z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def default_edges(B):
    return [125.0 * 2.0 ** (b - 0.5) for b in range(1, B)]


def band_of_bins(B, N, fs, edges=None):
    """[K] band index of every bin (-1: bins 0 and K/2 and above, which belong to no band), and K"""
    K = 1
    while K < N:
        K *= 2
    inner = default_edges(B) if edges is None else [float(np.float32(e)) for e in edges]
    bounds = [0.0] + inner + [fs / 2.0]
    k = np.arange(K, dtype=np.float64)
    f = k * float(fs) / float(K)
    band = np.full(K, -1, np.int64)
    for b in range(B):
        band[(f >= bounds[b]) & (f < bounds[b + 1])] = b
    band[0] = -1
    band[K // 2:] = -1
    return band, K


def carriers(B, N=48000, fs=48000, edges=None):
    """[B][N] float64 unit-power carriers"""
    band, K = band_of_bins(B, N, fs, edges)
    k = np.arange(K, dtype=np.uint64)
    phi = 2.0 * np.pi * (splitmix64(np.uint64(SEED) + k) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    out = np.empty((B, N))
    for b in range(B):
        X = np.where(band == b, np.exp(1j * phi), 0.0)
        r = (np.fft.ifft(X) * K).real[:N]
        out[b] = r * np.sqrt(N / np.sum(r * r))
    return out


def spectral_channel(env, c):
    B = env.shape[0]
    return np.sum(env.astype(np.float64) * c, axis=0) / np.sqrt(B)


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((a - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-300))


# ---- CPU ----

def test_flag_and_entry_point_are_exported(pkg):
    lib = pkg._capi.load()
    assert pkg._capi.FLAG_SPECTRAL_IR == FLAG
    assert "fs_set_band_edges" in pkg._capi.EXPORTS and hasattr(lib, "fs_set_band_edges")
    assert lib.fs_set_band_edges(None, None, 0) == pkg._capi.ERR_INVALID_ARGUMENT   # no context (no device needed)


def test_restated_carriers_invariants():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frequensee.h")).read()
    assert "#define FS_FLAG_SPECTRAL_IR 512u" in header                      # the definition restated here is the documented one
    assert "splitmix64(0x5EED + k) >> 40) 2^-24" in header and "125 * 2^(b - 0.5)" in header
    for B in (1, 4, 8):
        band, K = band_of_bins(B, 48000, 48000)
        assert K == 65536
        used = band[1:K // 2]
        assert (used >= 0).all() and np.array_equal(np.unique(used), np.arange(B))   # disjoint, covering [1, K/2)
        assert (np.diff(used) >= 0).all()
        c = carriers(B)
        assert np.allclose(np.mean(c * c, axis=1), 1.0, rtol=0, atol=1e-12)
    band, _ = band_of_bins(8, 48000, 48000)
    assert band[int(np.ceil(11313.708498984761 * 65536 / 48000))] == 7 and band[1] == 0


# ---- GPU ----

def ctx_with_source(pkg, B, **kw):
    ctx = pkg.Context(num_bands=B, **kw)
    return ctx, ctx.create_source(np.zeros(3, np.float32))


def spectral_params(pkg, **kw):
    flags = kw.pop("flags", 0)
    return pkg.default_params(flags=flags | FLAG, **kw)


@pytest.mark.gpu
def test_carrier_recovered_through_the_public_api(pkg):
    """A constant energy in one band makes env_b constant: the published IR is env_b c_b / sqrt(B)."""
    for B in (1, 4, 8):
        ctx, s = ctx_with_source(pkg, B)
        c = carriers(B)
        off = pkg.default_params()
        for edges in (None, [90.0 * 2.0 ** (b * 1.2) for b in range(B - 1)], "reset"):
            if edges == "reset":
                ctx.set_band_edges(None)
                c_now = c
            elif edges is not None:
                ctx.set_band_edges(edges)
                c_now = carriers(B, edges=edges)
            else:
                c_now = c
            for b in range(B):
                e = np.zeros((B, ctx.num_bins), np.float32)
                e[b] = 0.02
                ctx.update_energy_buffer(s, e)
                ctx.reconstruct_impulse_response(s, spectral_params(pkg))
                ir = ctx.impulse_response(s, 0)
                env = ctx.band_impulse_response(s, b)
                want = env.astype(np.float64) * c_now[b] / np.sqrt(B)
                assert np.abs(ir - want).max() <= 1e-4 * np.abs(want).max(), (B, edges, b)
                assert np.array_equal(ir, ctx.impulse_response(s, 1))
                ctx.reconstruct_impulse_response(s, off)   # without the flag: the constant positive envelope
                assert (ctx.impulse_response(s, 0) >= 0).all()
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,rays,div", [("starter_room", 4, 4096, 100.0), ("old_mine", 8, 65536, 1000.0)])
def test_exact_restatement_on_traced_frames(pkg, scene_factory, name, B, rays, div):
    sc = scene_factory(name, B)
    ctx = pkg.Context(num_bands=B)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    s = ctx.create_source(sc.source)
    c = carriers(B)
    for seed in (11, 12):
        p = pkg.default_params(num_rays=rays, depth=8, seed=seed, flags=DET, dist_divisor=div)
        ctx.compute_energy_response(s, p)
        ctx.reconstruct_impulse_response(s, pkg.default_params())
        plain = [ctx.band_impulse_response(s, b) for b in range(B)]
        ctx.reconstruct_impulse_response(s, spectral_params(pkg))
        env = np.array([ctx.band_impulse_response(s, b) for b in range(B)])
        for b in range(B):
            assert np.array_equal(env[b], plain[b]), b               # the band rows do not move
        assert np.abs(env).max() > 0
        ir = ctx.impulse_response(s, 0)
        assert rel_rms(ir, spectral_channel(env, c)) <= 1e-6
    ctx.close()


def band_power(y, band, K, B):
    Y = np.fft.rfft(np.asarray(y, np.float64), K)
    p = 2.0 * np.abs(Y[:K // 2]) ** 2 / K
    return np.array([p[band[:K // 2] == b].sum() for b in range(B)])


@pytest.mark.gpu
def test_spectrum_follows_absorption(pkg):
    """An absorption tilted from 0.05 (band 0) to 0.9 (band 7): band b's energy decays with a time constant ~ 1 / alpha_b
    (a direct-sound spike on top, the same in every band).  The published IR's power per band follows."""
    B = 8
    alpha = np.linspace(0.05, 0.9, B)
    ctx, s = ctx_with_source(pkg, B)
    i = np.arange(ctx.num_bins, dtype=np.float64)
    rng = np.random.default_rng(8)
    e = np.array([0.02 * np.exp(-(i - 4) / (60.0 * 0.05 / a)) * rng.uniform(0.5, 1.5, i.size) * (i >= 4) for a in alpha])
    e[:, 4] += 0.05
    ctx.update_energy_buffer(s, e.astype(np.float32))
    ctx.reconstruct_impulse_response(s, pkg.default_params())
    flat = ctx.impulse_response(s, 0)
    ctx.reconstruct_impulse_response(s, spectral_params(pkg))
    ir = ctx.impulse_response(s, 0)
    env = np.array([ctx.band_impulse_response(s, b) for b in range(B)], np.float64)
    band, K = band_of_bins(B, ctx.num_samples, 48000)
    want = np.sum(env * env, axis=1) / B                               # band b's energy in the IR
    got = band_power(ir, band, K, B)
    # the IR's spectrum is the definition's: band powers of the float64 restatement from the same band rows
    assert np.abs(10 * np.log10(got / band_power(spectral_channel(env, carriers(B)), band, K, B))).max() <= 0.05
    # and it follows the band energies: a band's power scatters around its energy by the carrier's own fluctuation under the
    # envelope (fixed carriers; the direct-sound spike lands on a few of their samples)
    wdb, gdb = 10 * np.log10(want), 10 * np.log10(got)
    assert wdb.max() - wdb.min() > 6.0, wdb
    assert np.corrcoef(wdb, gdb)[0, 1] >= 0.9, (wdb, gdb)
    # (this frame, measured: -0.8 / -3.5 dB in the two lowest bands, -1.7 .. +0.5 dB above 354 Hz — short of 3 / 1 dB)
    assert (np.abs(gdb - wdb)[:2] <= 4.0).all() and (np.abs(gdb - wdb)[2:] <= 2.0).all(), gdb - wdb
    assert got[7] < got[2]
    # the band-mean envelope has no such spectrum: its band powers are nowhere near the band energies
    flat_db = 10 * np.log10(np.maximum(band_power(flat, band, K, B), 1e-300) / want)
    assert np.abs(flat_db).max() > 10.0, flat_db
    ctx.close()


def seeded_frames(pkg, n, rays=8192):
    return [pkg.default_params(num_rays=rays, depth=8, seed=700 + i, flags=DET | FLAG, dist_divisor=100.0) for i in range(n)]


@pytest.mark.gpu
def test_every_route_gives_the_same_bits(pkg, scene_factory):
    sc = scene_factory("starter_room", 4)

    def fresh():
        ctx = pkg.Context(num_bands=4)
        ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
        ctx.set_listener(sc.listener)
        return ctx, ctx.create_source(sc.source)

    frames = seeded_frames(pkg, 6)
    ctx, s = fresh()                                   # synchronous compute + reconstruct
    want = []
    for p in frames:
        ctx.compute_energy_response(s, p)
        ctx.reconstruct_impulse_response(s, p)
        want.append(ctx.impulse_response(s, 0))
    assert np.abs(want[0]).max() > 0 and (want[0] < 0).any()   # broadband: both signs
    ctx.close()
    ctx, s = fresh()                                   # the tick
    for i, p in enumerate(frames):
        ctx.update_sources([s], p)
        assert np.array_equal(ctx.impulse_response(s, 0), want[i]), ("update_sources", i)
    ctx.close()
    ctx, s = fresh()                                   # the batched reconstruct
    for i, p in enumerate(frames):
        ctx.compute_energy_response_batch_async([s], p)
        ctx.reconstruct_impulse_response_batch_async([s], p)
        ctx.synchronize()
        assert np.array_equal(ctx.impulse_response(s, 0), want[i]), ("batch", i)
    ctx.close()
    for fpl in (1, 2):                                 # pipelined streams (fused reconstruct parts, published by the host word)
        ctx, s = fresh()
        ctx.set_pipelining(2)
        ctx.set_frames_per_launch(fpl)
        seen, stop = {}, threading.Event()
        lib, h = ctx.lib, ctx.h
        n = C.c_uint64()
        buf = np.empty(ctx.num_samples, np.float32)

        def reader():
            while not stop.is_set():
                lib.fs_get_impulse_response_sequence(h, s, C.byref(n))
                a = int(n.value)
                if a == 0 or a in seen:
                    continue
                lib.fs_copy_impulse_response(h, s, 0, buf.ctypes.data, buf.shape[0])
                lib.fs_get_impulse_response_sequence(h, s, C.byref(n))
                if int(n.value) == a:
                    seen[a] = buf.copy()

        t = threading.Thread(target=reader)
        t.start()
        try:
            for p in frames:
                ctx.compute_energy_response_async(s, p)
                ctx.reconstruct_impulse_response_async(s, p)
            ctx.synchronize()
        finally:
            stop.set()
            t.join()
        assert ctx.pipeline_counters()["publishes_by_word"] > 0
        assert np.array_equal(ctx.impulse_response(s, 0), want[-1]), ("stream", fpl)
        assert seen
        for a, ir in seen.items():
            assert np.array_equal(ir, want[a - 1]), ("reader", fpl, a)
        ctx.close()


@pytest.mark.gpu
def test_zero_block_rule_any_band(pkg):
    """Late bins with energy in ONE band (band mean below the 1e-6 cut, the band above it) after frames that filled or
    emptied those blocks: the kernel-written host slot equals the device row (a context whose reconstructs copy the whole
    row: profiling level 2 sends them through the tail stream's kernel + copy)."""
    B = 8
    masked, ms = ctx_with_source(pkg, B)
    copied, cs = ctx_with_source(pkg, B)
    copied.set_profiling(2)
    nb = masked.num_bins
    full = np.full((B, nb), 0.01, np.float32)
    small = np.zeros((B, nb), np.float32)
    small[:, :40] = 0.01
    small[3, 40:] = 5e-6                               # mean over the bands 6.25e-7 < 1e-6
    zero = np.zeros((B, nb), np.float32)
    zero[:, :40] = 0.01
    seq = [full, small, zero, small, full, small] * 2  # every transition of a slot's blocks (8 slots in the ring)
    p = spectral_params(pkg)
    for i, e in enumerate(seq):
        for ctx, s in ((masked, ms), (copied, cs)):
            ctx.update_energy_buffer(s, e)
            ctx.reconstruct_impulse_response(s, p)
        got, dev = masked.impulse_response(ms, 0), copied.impulse_response(cs, 0)
        assert np.array_equal(got, dev), i
        if e is small:
            assert np.abs(dev[45 * 49:]).max() > 0     # the late blocks are not zero
    masked.close(); copied.close()


@pytest.mark.gpu
def test_reverb_uses_the_spectral_ir(pkg):
    B = 4
    ctx, s = ctx_with_source(pkg, B)
    e = np.zeros((B, ctx.num_bins), np.float32)
    e[:, 2:300] = (0.05 * np.exp(-np.arange(298) / 60.0)).astype(np.float32)
    e[2] *= 0.2
    ctx.update_energy_buffer(s, e)
    ctx.reconstruct_impulse_response(s, spectral_params(pkg))
    ir = ctx.impulse_response(s, 0).astype(np.float64)
    assert (ir < 0).any()
    ctx.reverb_init(s, FRAME)
    rng = np.random.default_rng(4)
    hist = np.zeros((2, 47999 + FRAME), np.float64)
    for _ in range(4):
        blk = np.clip(rng.normal(0, 0.3, 2 * FRAME), -1, 1).astype(np.float32)
        y = ctx.reverb_process(s, blk)
        for ch in range(2):
            hist[ch] = np.concatenate([hist[ch][FRAME:], blk[ch::2].astype(np.float64)])
            want = np.array([np.dot(ir, hist[ch][t:t + 48000][::-1]) for t in range(FRAME)])
            assert np.abs(y[ch::2] - np.clip(want, -1, 1)).max() < 5e-5 * max(1.0, np.abs(want).max())
    ctx.close()


@pytest.mark.gpu
def test_band_edge_validation(pkg):
    B = 8
    ctx, s = ctx_with_source(pkg, B)
    good = default_edges(B)
    ctx.set_band_edges(good)
    f = 1000 * 48000 / 65536                                         # bin 1000 (bins are 0.73 Hz apart)
    for bad in (good[:-1],                                           # a wrong count
                good[::-1],                                          # descending
                good[:-1] + [24000.0],                               # an edge at Nyquist
                [0.0] + good[1:], [-5.0] + good[1:],                 # an edge <= 0
                good[:2] + [f + 0.05, f + 0.15] + good[4:]):         # two edges closer than one bin: band 2 gets none
        with pytest.raises(pkg.FrequenSeeError) as ei:
            ctx.set_band_edges(bad)
        assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT and "fs_set_band_edges" in str(ei.value)
    ctx.set_band_edges(None)
    ctx.close()
    ctx, s = ctx_with_source(pkg, B, sample_rate=16000)
    ctx.update_energy_buffer(s, np.full((B, ctx.num_bins), 0.01, np.float32))
    with pytest.raises(pkg.FrequenSeeError) as ei:
        ctx.reconstruct_impulse_response(s, spectral_params(pkg))
    assert "fs_set_band_edges" in str(ei.value)
    ctx.reconstruct_impulse_response(s, pkg.default_params())      # without the flag: as before
    ctx.set_band_edges([100.0 * 2 ** b for b in range(B - 1)])     # (up to 6 400 Hz < 8 000)
    ctx.reconstruct_impulse_response(s, spectral_params(pkg))
    assert (ctx.impulse_response(s, 0) < 0).any()
    ctx.close()
