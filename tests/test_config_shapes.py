"""The kernels at context shapes other than the default one (1 000 bins, 48 000 samples, 49 samples per bin).

Sample rate, simulated duration and bin duration of fs_config set the size of everything the kernels index: the connect
deposit's clamp bin and LDS window, the reconstruct's 16-sample chunks and 4 096-sample blocks, the zero-block masks of
the host ring slots (used up to 32 blocks), the spectral carriers' FFT length, the reverb's history ring.  Each shape
below is traced and reconstructed and checked against the CPU oracle and a float64 numpy restatement of
ReconstructImpulseResponse (FSAC.cpp:320-380).  num_bins and num_samples are always read back from the context: float
ceil decides them (FSAC.h:137-138), and the CPU part at the end restates that rule for every shape.
"""
import re

import numpy as np
import pytest

from test_gpu_parity import IR_TOL, TIGHT_TOL, check_energy, rel_rms
from test_spectral_ir import carriers, spectral_channel

DET = 8            # FS_FLAG_DETERMINISTIC
SPECTRAL = 512     # FS_FLAG_SPECTRAL_IR
BLOCK = 4096       # samples per reconstruct workgroup (kReconBlockSamples)

# id -> (sample_rate, simulated_duration, bin_duration)
SHAPES = {
    "sr44100": (44100, 1.0, 0.001),          # 44 100 samples: partial last chunk and block; 45 samples per bin, nb * spb > ns
    "sr22050_bin2ms": (22050, 1.0, 0.002),   # 500 bins while deposits use 1 ms bins: the clamp bin collects the late paths
    "short_250ms": (48000, 0.25, 0.001),     # fewer bins than the LDS window: all of the histogram in LDS
    "tiny_20ms": (48000, 0.02, 0.001),       # 960 samples, less than one block; most deposits in the clamp bin
    "one_bin": (48000, 0.5, 0.5),            # nb = 1
    "ten_samples": (10, 1.0, 0.001),         # 10 samples, 1 sample per bin, 990 bins beyond the IR
    "sr96000": (96000, 0.5, 0.001),          # 97 samples per bin
    "masks_32": (48000, 2.7, 0.001),         # 129 600 samples = 32 blocks: the last bit of the mask word
    "masks_off": (48000, 2.75, 0.001),       # 132 000 samples = 33 blocks: no masks
}
DEFAULT = (48000, 1.0, 0.001)


def cfg(shape):
    sr, dur, bd = SHAPES[shape] if shape != "default" else DEFAULT
    return dict(sample_rate=sr, simulated_duration=dur, bin_duration=bd)


def spb_of(shape):
    """FSAC.cpp:324 in float32: CeilToInt(BinDuration * SampleRate)"""
    c = cfg(shape)
    return int(np.ceil(np.float32(c["bin_duration"]) * np.float32(c["sample_rate"])))


def slow_sound(shape):
    """a sound speed at which starter_room's paths (12 m and longer at dist_divisor 100) spread over the IR and beyond it: at 1 s,
    deposits in bins 124 - 999, in the default LDS window, beyond it and in the clamp bin (the slow_sound_late_bins variant of
    test_gpu_parity.py, scaled to the duration)"""
    return 100.0 / cfg(shape)["simulated_duration"]


def new_ctx(pkg, sc, shape, B, nsrc=1, **kw):
    ctx = pkg.Context(num_bands=B, **cfg(shape), **kw)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    return ctx, [ctx.create_source(p) for p in source_positions(sc, nsrc)]


def source_positions(sc, n):
    rng = np.random.default_rng(n)
    lo, hi = sc.triangles.min(axis=(0, 1)), sc.triangles.max(axis=(0, 1))
    return [np.asarray(sc.source, np.float32)] + [(sc.source + rng.uniform(-0.1, 0.1, 3) * (hi - lo)).astype(np.float32)
                                                   for _ in range(n - 1)]


def gpu_params(pkg, shape, rays, seed, speed=None, gain=1.0, **kw):
    return pkg.default_params(num_rays=rays, depth=8, seed=seed, dist_divisor=100.0, sound_speed=speed or slow_sound(shape),
                              energy_gain=gain, **kw)


_oracle_cache = {}


def oracle_energy(oracle_mod, sc, shape, num_bins, rays, seed, pos=None, threads=0, speed=None, gain=1.0):
    """(e32, e64, counters) of the oracle for the frame gpu_params describes (flags other than deterministic mode do not occur here)"""
    pos = sc.source if pos is None else pos
    speed = speed or slow_sound(shape)
    key = (sc.name, sc.num_bands, shape, num_bins, rays, seed, speed, gain, tuple(np.asarray(pos, np.float32).tolist()))
    if key not in _oracle_cache:
        osc = oracle_mod.Scene(sc.triangles, sc.material_ids, sc.absorption)
        op = oracle_mod.default_params(num_pairs=rays // 2, depth=8, seed=seed, dist_divisor=100.0, sound_speed=speed, energy_gain=gain)
        if threads:
            _oracle_cache[key] = osc.compute_energy_mt(op, pos, sc.listener, threads, num_bins=num_bins)
        else:
            _oracle_cache[key] = osc.compute_energy(op, pos, sc.listener, num_bins=num_bins)
    return _oracle_cache[key]


def check_energy_det(got, e32, e64, B):
    """check_energy for deterministic mode, which sums integer quanta of 2^-40 (fs_dev_common.hpp: kFixedScale): a deposit below half
    a quantum rounds to nothing, so only bins the oracle fills well above the quantum must be occupied (the frames here use a
    gain of 1e6 so that the quanta are far below the energies that matter)"""
    assert not got[e32 == 0].any()                                      # no bin the oracle leaves empty
    assert (got != 0)[e64 >= 1e-9].all()
    for b in range(B):
        assert rel_rms(got[b], e64[b]) <= TIGHT_TOL, b


def check_counters(ctx, cnt):
    st = ctx.stats()
    assert (st["segments"], st["connections_tested"], st["deposits"]) == (cnt.closest_rays, cnt.any_rays, cnt.connected)


# ---- the float64 restatement of ReconstructImpulseResponse ------------------------------------------------------------------
_FILTER_TAPS = 0.25 * 0.75 ** np.arange(320)   # 0.75^320 ~ 1e-40: the one-pole filter's impulse response, exact to float64


def reconstruct_f64(energy, num_samples, samples_per_bin):
    """FSAC.cpp:320-380 for one fp32 energy row (tests/test_independent_restatement.py, vectorised): the amplitude of every bin
    (:343-345), linear interpolation from the previous bin's amplitude (:347-362) over samples_per_bin samples per bin — samples
    beyond the last bin stay zero (:335, :340) — and the one-pole filter y[i] = 0.25 x[i] + 0.75 y[i-1], y[0] = x[0] (:366-375),
    evaluated as x * h + 0.75^(i+1) x[0] (the initial condition y[-1] = x[0])."""
    e32 = np.asarray(energy, np.float32)
    e = e32.astype(np.float64)
    amp = np.zeros_like(e)
    ok = np.abs(e32) >= np.float32(1e-6)                                    # :343 (a float comparison)
    amp[ok] = e[ok] / np.sqrt(e[ok] * np.sqrt(4.0 * np.pi))                # :345
    i = np.arange(num_samples)
    b = i // samples_per_bin
    w = (i - b * samples_per_bin) / samples_per_bin                         # :359
    inside = b < e.size
    bc = np.minimum(b, e.size - 1)
    cur = amp[bc]
    prev = np.where(bc == 0, amp[0], amp[np.maximum(bc - 1, 0)])            # :347-355
    x = np.where(inside, (1.0 - w) * prev + w * cur, 0.0)                   # :360
    y = np.convolve(x, _FILTER_TAPS)[:num_samples]
    y += 0.75 ** (i + 1.0) * x[0]
    return y


def band_mean(e):
    """the channel view's energy: the band mean in fp32, summed band after band (FSAC.cpp:331 over the bands)"""
    e = np.asarray(e, np.float32)
    s = e[0].copy()
    for row in e[1:]:
        s = (s + row).astype(np.float32)
    return (s / np.float32(e.shape[0])).astype(np.float32)


def check_ir(got, energy_row, num_samples, spb, oracle_mod, shape, spb_override=0, what=""):
    """got against the float64 restatement and the oracle's fp32 reconstruct, both within IR_TOL of the peak"""
    want = reconstruct_f64(energy_row, num_samples, spb)
    peak = max(np.abs(want).max(), 1e-30)
    assert got.shape == (num_samples,)
    err = np.abs(got.astype(np.float64) - want)
    assert err.max() <= IR_TOL * peak, (what, int(np.argmax(err)), float(err.max() / peak))
    c = cfg(shape)
    ref = oracle_mod.reconstruct(energy_row, sample_rate=c["sample_rate"], bin_duration=c["bin_duration"],
                                 num_samples=num_samples, samples_per_bin=spb_override)
    assert np.abs(got - ref).max() <= IR_TOL * peak, what


def synthetic_energy(rng, B, nb):
    """every bin occupied (every sample of the IR non-zero), with empty bins and bins under the 1e-6 amplitude cut among them"""
    e = (rng.random((B, nb)) * 0.02 + 1e-4).astype(np.float32)
    if nb >= 8:
        e[:, rng.integers(0, nb, nb // 7)] = 0.0
        e[:, rng.integers(0, nb, nb // 8)] = 5e-7
    return e


# ==== GPU ===================================================================================================================

# ---- 1. energy against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_energy_matches_the_oracle(pkg, oracle_mod, scene_factory, shape, B):
    sc = scene_factory("starter_room", B)
    ctx, (s,) = new_ctx(pkg, sc, shape, B)
    nb = ctx.num_bins
    rays = 8192
    ctx.reset_stats()
    got = ctx.compute_energy_response(s, gpu_params(pkg, shape, rays, 0x5EED + B))
    e32, e64, cnt = oracle_energy(oracle_mod, sc, shape, nb, rays, 0x5EED + B)
    assert cnt.connected > 0 and e32[:, nb - 1].any()                  # the clamp bin is reached
    check_counters(ctx, cnt)
    check_energy(got, e32, e64, B)
    ctx.close()


@pytest.mark.gpu
def test_energy_large_frame_sr44100(pkg, oracle_mod, scene_factory):
    """one 262 144-ray frame (walks and connects on the whole chip, deposits from many workgroups into every part of the histogram)"""
    shape, B, rays = "sr44100", 8, 262144
    sc = scene_factory("starter_room", B)
    ctx, (s,) = new_ctx(pkg, sc, shape, B)
    ctx.reset_stats()
    got = ctx.compute_energy_response(s, gpu_params(pkg, shape, rays, 41))
    e32, e64, cnt = oracle_energy(oracle_mod, sc, shape, ctx.num_bins, rays, 41, threads=8)
    check_counters(ctx, cnt)
    assert np.array_equal(got != 0, e64 != 0)
    for b in range(B):
        assert rel_rms(got[b], e64[b]) <= TIGHT_TOL, b
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["sr44100", "masks_off"])
def test_deterministic_energy(pkg, oracle_mod, scene_factory, shape):
    B, rays = 3, 8192
    sc = scene_factory("starter_room", B)
    ctx, (s,) = new_ctx(pkg, sc, shape, B)
    p = gpu_params(pkg, shape, rays, 7, gain=1e6, flags=DET)
    ctx.reset_stats()
    got = ctx.compute_energy_response(s, p).copy()
    e32, e64, cnt = oracle_energy(oracle_mod, sc, shape, ctx.num_bins, rays, 7, gain=1e6)
    check_counters(ctx, cnt)
    check_energy_det(got, e32, e64, B)
    assert np.array_equal(ctx.compute_energy_response(s, p), got)      # the same bits again
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["short_250ms", "sr44100"])
def test_batched_sources_energy(pkg, oracle_mod, scene_factory, shape):
    """three sources in one traced frame (the energy tables are laid out with a stride of nb): each matches its own oracle frame"""
    B, rays = 3, 4096
    sc = scene_factory("starter_room", B)
    ctx, srcs = new_ctx(pkg, sc, shape, B, nsrc=3)
    pos = source_positions(sc, 3)
    for flags, gain, check in ((0, 1.0, check_energy), (DET, 1e6, check_energy_det)):
        ctx.reset_stats()
        ctx.compute_energy_response_batch_async(srcs, gpu_params(pkg, shape, rays, 9, gain=gain, flags=flags))
        ctx.synchronize()
        tot = [0, 0, 0]
        for i, s in enumerate(srcs):
            e32, e64, cnt = oracle_energy(oracle_mod, sc, shape, ctx.num_bins, rays, 9, pos=pos[i], gain=gain)
            check(ctx.energy_buffer(s), e32, e64, B)
            tot = [tot[0] + cnt.closest_rays, tot[1] + cnt.any_rays, tot[2] + cnt.connected]
        st = ctx.stats()
        assert [st["segments"], st["connections_tested"], st["deposits"]] == tot
    ctx.close()


# ---- 2. impulse responses against the restatement --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 2, 5])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_impulse_responses_match_the_restatement(pkg, oracle_mod, shape, channels):
    B = 3
    ctx = pkg.Context(num_bands=B, num_channels=channels, **cfg(shape))
    s = ctx.create_source((0.0, 0.0, 0.0))
    nb, ns, spb = ctx.num_bins, ctx.num_samples, spb_of(shape)
    rng = np.random.default_rng(ns + channels)
    for rep in range(2):                                                # a second energy over the first: nothing of it stays
        e = synthetic_energy(rng, B, nb)
        ctx.update_energy_buffer(s, e)
        ctx.reconstruct_impulse_response(s)
        for b in range(B):
            check_ir(ctx.band_impulse_response(s, b), e[b], ns, spb, oracle_mod, shape, what=("band", b, rep))
        ch0 = ctx.impulse_response(s, 0)
        check_ir(ch0, band_mean(e), ns, spb, oracle_mod, shape, what=("channel", rep))
        assert ch0[-1] != 0.0                                           # the last sample is written
        for c in range(1, channels):
            assert np.array_equal(ctx.impulse_response(s, c), ch0), c
        with pytest.raises(pkg.FrequenSeeError):
            ctx.impulse_response(s, channels)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["default", "sr44100"])
def test_samples_per_bin_overrides(pkg, oracle_mod, shape):
    """fs_params.samples_per_bin: 1, 7, 4 097 (a bin longer than a block) and 32 767 (a bin longer than the IR)"""
    B = 3
    ctx = pkg.Context(num_bands=B, **cfg(shape))
    s = ctx.create_source((0.0, 0.0, 0.0))
    nb, ns = ctx.num_bins, ctx.num_samples
    e = synthetic_energy(np.random.default_rng(3), B, nb)
    ctx.update_energy_buffer(s, e)
    for spb in (1, 7, 4097, 32767):
        ctx.reconstruct_impulse_response(s, pkg.default_params(samples_per_bin=spb))
        for b in range(B):
            check_ir(ctx.band_impulse_response(s, b), e[b], ns, spb, oracle_mod, shape, spb_override=spb, what=(spb, b))
        check_ir(ctx.impulse_response(s, 0), band_mean(e), ns, spb, oracle_mod, shape, spb_override=spb, what=(spb, "channel"))
    ctx.close()


# ---- 3. every route publishes the same bits --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["sr44100", "masks_32", "masks_off"])
def test_every_route_publishes_the_same_bits(pkg, scene_factory, shape):
    """the synchronous reconstruct, the batch reconstruct, update_sources and a pipelined stream (fused reconstruct parts) over
    three sources and deterministic frames: bit-identical published IRs and band IRs"""
    B, rays = 3, 4096
    sc = scene_factory("starter_room", B)
    frames = [gpu_params(pkg, shape, rays, 300 + i, gain=1e6, flags=DET) for i in range(2)]   # (gain: amplitudes over several blocks)

    def run(route):
        ctx, srcs = new_ctx(pkg, sc, shape, B, nsrc=3)
        if route == "stream":
            ctx.set_pipelining(2)
            ctx.set_frames_per_launch(2)
        for p in frames:
            if route == "sync":
                for s in srcs:
                    ctx.compute_energy_response(s, p)
                    ctx.reconstruct_impulse_response(s, p)
            elif route == "batch":
                ctx.compute_energy_response_batch_async(srcs, p)
                ctx.reconstruct_impulse_response_batch_async(srcs, p)
            elif route == "update_sources":
                ctx.update_sources(srcs, p)
            else:
                for s in srcs:
                    ctx.compute_energy_response_async(s, p)
                    ctx.reconstruct_impulse_response_async(s, p)
                ctx.submit()
        ctx.synchronize()
        out = [(ctx.impulse_response(s, 0), ctx.impulse_response(s, 1), [ctx.band_impulse_response(s, b) for b in range(B)],
                ctx.energy_buffer(s)) for s in srcs]
        if route == "stream":
            assert ctx.pipeline_counters()["publishes_by_word"] > 0
        ctx.close()
        return out

    want = run("sync")
    for i, (ir, ir1, bands, e) in enumerate(want):
        assert np.array_equal(ir, ir1)
        assert sum(np.abs(ir[k:k + BLOCK]).max() > 0 for k in range(0, ir.size, BLOCK)) >= 2   # non-zero in several blocks
        want_ir = reconstruct_f64(band_mean(e), ir.size, spb_of(shape))
        assert np.abs(ir - want_ir).max() <= IR_TOL * np.abs(want_ir).max(), i
    for route in ("batch", "update_sources", "stream"):
        got = run(route)
        for i in range(3):
            assert np.array_equal(got[i][3], want[i][3]), (route, i, "energy")
            assert np.array_equal(got[i][0], want[i][0]), (route, i, "channel 0")
            assert np.array_equal(got[i][1], want[i][1]), (route, i, "channel 1")
            for b in range(B):
                assert np.array_equal(got[i][2][b], want[i][2][b]), (route, i, "band", b)


# ---- 4. zero blocks of the host ring slots ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["masks_32", "masks_off"])
def test_zero_blocks_at_32_and_33_blocks(pkg, shape):
    """test_round5.py's alternation of late-bin and early-bin energies (runs longer and shorter than the 8-slot ring) at the
    largest shape with zero-block masks (mask bit 31 in use) and the smallest without: every published IR equals the one a fresh
    context produces for the same energy"""
    B = 3
    ctx = pkg.Context(num_bands=B, **cfg(shape))
    src = ctx.create_source((0.0, 0.0, 0.0))
    nb, ns = ctx.num_bins, ctx.num_samples
    nblocks = (ns + BLOCK - 1) // BLOCK
    assert nblocks == (32 if shape == "masks_32" else 33)
    rng = np.random.default_rng(nblocks)
    last = (ns - 1) // spb_of(shape) - 1                                # a bin of the last block (bins from ns / spb on are not in the IR)

    def energy(kind):
        e = np.zeros((B, nb), np.float32)
        if kind == "late":
            e[:, rng.integers(0, nb, 60)] = rng.random(60).astype(np.float32) + 0.1
            e[:, [last, nb - 1]] = 0.5                                  # the last block (bit 31, or block 32) and the clamp bin
        elif kind == "early":
            e[:, rng.integers(0, 30, 10)] = rng.random(10).astype(np.float32) + 0.1
        elif kind == "middle":
            e[:, nb // 2 + rng.integers(0, 50, 10)] = rng.random(10).astype(np.float32) + 0.1
        elif kind == "last":                                            # only the last block and the first
            e[:, [3, last]] = 0.3
        return e

    def fresh_ir(e):
        ref = pkg.Context(num_bands=B, **cfg(shape))
        rs = ref.create_source((0.0, 0.0, 0.0))
        ref.update_energy_buffer(rs, e)
        ref.reconstruct_impulse_response(rs)
        out = ref.impulse_response(rs, 0)
        ref.close()
        return out

    seq = ["late"] * 3 + ["early"] * 9 + ["zero"] * 2 + ["middle"] * 9 + ["late"] * 9 + ["last"] * 3 + ["early"] * 3 + \
        ["set"] + ["last"] * 9 + ["late"] * 2 + ["zero"] * 9
    for i, kind in enumerate(seq):
        if kind == "set":                                               # a copy command rewrites a whole slot
            ir = rng.random(ns).astype(np.float32) - 0.5
            ctx.set_impulse_response(src, ir)
            assert np.array_equal(ctx.impulse_response(src, 0), ir)
            continue
        e = energy(kind)
        ctx.update_energy_buffer(src, e)
        ctx.reconstruct_impulse_response(src)
        got = ctx.impulse_response(src, 0)
        want = fresh_ir(e)
        assert np.array_equal(got, want), (i, kind, int(np.flatnonzero(got != want)[0]))
        if kind == "early":
            assert not got[BLOCK:].any()
        if kind in ("late", "last"):
            assert got[(nblocks - 1) * BLOCK:].any()
    ctx.close()


# ---- 5. spectral impulse responses: carriers of K = next_pow2(ns) != ns --------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["sr44100", "sr96000"])
def test_spectral_restatement(pkg, scene_factory, shape):
    B, rays = 4, 8192
    sc = scene_factory("starter_room", B)
    ctx, (s,) = new_ctx(pkg, sc, shape, B)
    ns, sr = ctx.num_samples, cfg(shape)["sample_rate"]
    c = carriers(B, N=ns, fs=sr)
    for seed in (21, 22):
        ctx.compute_energy_response(s, gpu_params(pkg, shape, rays, seed, flags=DET))
        ctx.reconstruct_impulse_response(s, pkg.default_params())
        plain = [ctx.band_impulse_response(s, b) for b in range(B)]
        ctx.reconstruct_impulse_response(s, pkg.default_params(flags=SPECTRAL))
        env = np.array([ctx.band_impulse_response(s, b) for b in range(B)])
        for b in range(B):
            assert np.array_equal(env[b], plain[b]), b
        ir = ctx.impulse_response(s, 0)
        assert np.abs(env).max() > 0 and (ir < 0).any()
        assert rel_rms(ir, spectral_channel(env, c)) <= 1e-6
        assert np.array_equal(ir, ctx.impulse_response(s, 1))
    ctx.close()


# ---- 6. AddEnergyAtDelay at 20 bins ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_add_energy_at_delay_tiny(pkg, oracle_mod):
    from test_independent_restatement import bin_of
    B = 3
    ctx = pkg.Context(num_bands=B, **cfg("tiny_20ms"))
    s = ctx.create_source((0.0, 0.0, 0.0))
    nb = ctx.num_bins
    assert nb == 20
    ctx.check(ctx.lib.fs_flush_energy_buffer(ctx.h, s))
    want = np.zeros((B, nb), np.float32)
    for k, delay in enumerate((-1.0, 0.0, 0.0199, 0.02, 5.0)):
        for b in range(B):
            e = float(np.float32(0.1 * (k + 1) + 0.01 * b))
            ctx.check(ctx.lib.fs_add_energy_at_delay(ctx.h, s, b, delay, e))
            bin_ = oracle_mod.add_energy_at_delay(want[b], delay, e)
            assert bin_ == bin_of(delay, num_bins=nb), delay
    assert np.array_equal(ctx.energy_buffer(s), want)
    assert want[:, nb - 1].any() and want[:, 0].any()
    ctx.close()


# ---- 7. the connect part's LDS window --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("window", [1, 16, 4096])
def test_hist_window_override(pkg, oracle_mod, scene_factory, monkeypatch, window, B):
    """FS_HIST_WINDOW (read at fs_context_create): the first W bins of the histogram in LDS, the rest through global atomics —
    1 (every deposit but bin 0 far), 16, 4 096 (clamped to nb: all in LDS).  Oracle parity, and under deterministic mode the same
    bits as the default window."""
    shape, rays = "default", 8192
    sc = scene_factory("starter_room", B)
    monkeypatch.setenv("FS_HIST_WINDOW", str(window))
    ctx, (s,) = new_ctx(pkg, sc, shape, B)
    monkeypatch.delenv("FS_HIST_WINDOW")
    ref, (rs,) = new_ctx(pkg, sc, shape, B)
    for speed, lo, hi in ((2000.0, 1, 16), (100.0, 256, ctx.num_bins - 1)):   # deposits in bins 6 - 51, and 124 - 999
        ctx.reset_stats()
        got = ctx.compute_energy_response(s, gpu_params(pkg, shape, rays, 0x5EED + B, speed=speed)).copy()
        e32, e64, cnt = oracle_energy(oracle_mod, sc, shape, ctx.num_bins, rays, 0x5EED + B, speed=speed)
        check_counters(ctx, cnt)
        check_energy(got, e32, e64, B)
        assert (e32[:, lo:] != 0).any() and (e32[:, :hi] != 0).any()   # deposits on both sides of a window edge
        p = gpu_params(pkg, shape, rays, 0x5EED + B, speed=speed, flags=DET)
        assert np.array_equal(ctx.compute_energy_response(s, p), ref.compute_energy_response(rs, p))
        # the batched frame's connect part as well
        ctx.compute_energy_response_batch_async([s], p)
        ref.compute_energy_response_batch_async([rs], p)
        ctx.synchronize(); ref.synchronize()
        assert np.array_equal(ctx.energy_buffer(s), ref.energy_buffer(rs))
    ctx.close(); ref.close()


# ---- 8. the reverb convolution at other IR lengths and frame sizes ---------------------------------------------------------
def conv_f64(x, h, n):
    """the first n samples of the linear convolution x * h in float64"""
    if min(len(x), len(h)) <= 512:
        return np.convolve(x, h)[:n]
    L = 1
    while L < len(x) + len(h):
        L *= 2
    return np.fft.irfft(np.fft.rfft(x, L) * np.fft.rfft(h, L), L)[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [1, 15, 17, 480, 16384])
@pytest.mark.parametrize("ir_len", [12000, 44100, 65537])
def test_reverb_convolution(pkg, ir_len, frame):
    """RVB.cpp:118-170 with an IR of ir_len samples (a 1 s context at ir_len Hz): out[t] = sum_k IR[k] u[t - k], clamped, both
    channels.  The callbacks alternate the literal tail off and on (the history ring holds the true samples either way) and go on
    until the 65 536-sample history ring has wrapped (frame 1: 3 000 callbacks, the ring does not wrap)."""
    ctx = pkg.Context(num_bands=1, sample_rate=ir_len, simulated_duration=1.0)
    s = ctx.create_source((0.0, 0.0, 0.0))
    assert ctx.num_samples == ir_len
    rng = np.random.default_rng(ir_len + frame)
    n = np.arange(ir_len)
    ir = (rng.normal(0, 1, ir_len) * np.exp(-n / (ir_len / 3.0)) * 0.004).astype(np.float32)
    ir[0] = 0.25
    ir[-1] = 0.1                                                        # the oldest tap reads the far end of the ring
    ctx.set_impulse_response(s, ir)
    ctx.reverb_init(s, frame)
    calls = 3000 if frame == 1 else 65536 // frame + max(3, 4096 // frame)
    x = np.clip(rng.normal(0, 0.3, (calls, 2 * frame)), -1, 1).astype(np.float32)
    y = np.empty_like(x)
    for c in range(calls):
        y[c] = ctx.reverb_process(s, x[c], literal_tail=bool(c % 2))
    h = ir.astype(np.float64)
    for ch in range(2):
        stream = x[:, ch::2].astype(np.float64).reshape(-1)
        want = conv_f64(stream, h, stream.size).reshape(calls, frame)
        for c in range(1, calls, 2):   # RVB.cpp:147-148: the current block is the interleaved buffer's first `frame` floats
            d = x[c, :frame].astype(np.float64) - x[c, ch::2].astype(np.float64)
            want[c] += conv_f64(d, h[:frame], frame)
        want = np.clip(want, -1.0, 1.0)
        err = np.abs(y[:, ch::2] - want)
        assert err.max() <= 5e-5 * max(1.0, np.abs(want).max()), (ch, np.unravel_index(np.argmax(err), err.shape))
    ctx.reverb_release(s)                                               # ClearBuffers: silence in, silence out
    assert not ctx.reverb_process(s, np.zeros(2 * frame, np.float32)).any()
    ctx.close()


@pytest.mark.gpu
def test_reverb_refuses_an_ir_longer_than_the_ring(pkg):
    ctx = pkg.Context(num_bands=1, sample_rate=65538, simulated_duration=1.0)
    s = ctx.create_source((0.0, 0.0, 0.0))
    assert ctx.num_samples == 65538
    with pytest.raises(pkg.FrequenSeeError) as ei:
        ctx.reverb_init(s, 1024)
    assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    ctx.close()


# ---- the reconstruct's LDS: the largest accepted shape works, the next one is refused -------------------------------------
def duration_for_bins(oracle_mod, nb, bin_duration):
    """a float32 simulated_duration that gives exactly nb bins by the library's rule (FSAC.h:137)"""
    lib = oracle_mod.load()
    d = np.float32(nb * bin_duration)
    for _ in range(64):
        got = lib.fso_num_bins(float(d), bin_duration)
        if got == nb:
            return float(d)
        d = np.nextafter(d, np.float32(np.inf if got < nb else -np.inf), dtype=np.float32)
    raise AssertionError(nb)


@pytest.mark.gpu
def test_lds_edge(pkg, oracle_mod, scene_factory):
    """fs_context_create accepts exactly the shapes whose reconstruct fits the device's LDS per workgroup (recon_lds_bytes:
    4 (nb + 4 096 + 96 + 256 x 17) bytes, and 4 096 bytes more for the static LDS of the kernels that carry a reconstruct).  The largest one traces, reconstructs on every route and matches the oracle and the
    restatement; one bin more is refused with FS_ERR_INVALID_ARGUMENT."""
    with pytest.raises(pkg.FrequenSeeError) as ei:
        pkg.Context(num_bands=1, sample_rate=8000, simulated_duration=1000.0)      # a million bins
    assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    m = re.search(r"the device offers (\d+) \(at most (\d+) bins\)", str(ei.value))
    assert m, str(ei.value)
    lds, nmax = int(m.group(1)), int(m.group(2))
    need = lambda nb: 4 * (nb + 4096 + 96 + 256 * 17) + 4096        # recon_lds_bytes + room for the kernels' static LDS
    assert need(nmax) <= lds < need(nmax + 1)
    bd = 0.001
    with pytest.raises(pkg.FrequenSeeError) as ei:
        pkg.Context(num_bands=1, sample_rate=8000, simulated_duration=duration_for_bins(oracle_mod, nmax + 1, bd), bin_duration=bd)
    assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT and "LDS" in str(ei.value)

    B, rays, shape = 1, 4096, "lds_edge"
    SHAPES[shape] = (8000, duration_for_bins(oracle_mod, nmax, bd), bd)
    try:
        sc = scene_factory("starter_room", B)
        ctx, srcs = new_ctx(pkg, sc, shape, B, nsrc=2)
        nb, ns, spb = ctx.num_bins, ctx.num_samples, spb_of(shape)
        assert nb == nmax
        p = gpu_params(pkg, shape, rays, 5, gain=1e6, flags=DET)
        ctx.reset_stats()
        got = ctx.compute_energy_response(srcs[0], p).copy()
        e32, e64, cnt = oracle_energy(oracle_mod, sc, shape, nb, rays, 5, gain=1e6)
        check_counters(ctx, cnt)
        check_energy_det(got, e32, e64, B)
        ctx.reconstruct_impulse_response(srcs[0], p)
        want = ctx.impulse_response(srcs[0], 0)
        check_ir(want, got[0], ns, spb, oracle_mod, shape, what="sync")
        # the batch kernel, and the fused frame kernel's reconstruct parts (plain and spectral) of a pipelined stream
        e = synthetic_energy(np.random.default_rng(1), B, nb)
        ctx.update_energy_buffer(srcs[1], e)
        ctx.reconstruct_impulse_response_batch_async(srcs[1:], p)
        ctx.synchronize()
        check_ir(ctx.impulse_response(srcs[1], 0), e[0], ns, spb, oracle_mod, shape, what="batch")
        ctx.set_pipelining(2)
        ctx.set_frames_per_launch(2)
        for flags in (DET, DET | SPECTRAL):
            q = gpu_params(pkg, shape, rays, 5, gain=1e6, flags=flags)
            for s in srcs:
                ctx.compute_energy_response_async(s, q)
                ctx.reconstruct_impulse_response_async(s, q)
            ctx.submit()
            ctx.synchronize()
            for s in srcs:
                ir = ctx.impulse_response(s, 0)
                if flags & SPECTRAL:
                    env = ctx.band_impulse_response(s, 0)
                    assert rel_rms(ir, spectral_channel(env[None], carriers(1, N=ns, fs=8000))) <= 1e-6
                else:
                    check_ir(ir, ctx.energy_buffer(s)[0], ns, spb, oracle_mod, shape, what=("stream", s))
        assert np.array_equal(ctx.impulse_response(srcs[0], 1), ctx.impulse_response(srcs[0], 0))
        ctx.close()
    finally:
        del SHAPES[shape]


# ==== CPU: the shapes themselves ============================================================================================
@pytest.mark.parametrize("shape", list(SHAPES) + ["default"])
def test_shape_sizes_restated_in_float32(oracle_mod, shape):
    """fso_num_bins / fso_num_samples / fso_samples_per_bin (the library's rule) against FSAC.h:137-138 and FSAC.cpp:324 restated
    in float32 numpy, and each shape is what the GPU tests above rely on"""
    c = cfg(shape)
    lib = oracle_mod.load()
    f32 = np.float32
    dur, bd, sr = f32(c["simulated_duration"]), f32(c["bin_duration"]), f32(c["sample_rate"])
    nb = int(np.ceil(dur / bd))
    ns = int(np.ceil(dur * sr))
    spb = int(np.ceil(bd * sr))
    assert lib.fso_num_bins(c["simulated_duration"], c["bin_duration"]) == nb
    assert lib.fso_num_samples(c["simulated_duration"], c["sample_rate"]) == ns
    assert lib.fso_samples_per_bin(c["bin_duration"], c["sample_rate"]) == spb == spb_of(shape)
    expect = {
        "default": (1000, 48000, 49), "sr44100": (1000, 44100, 45), "sr22050_bin2ms": (500, 22050, 45),
        "short_250ms": (250, 12000, 49), "tiny_20ms": (20, 960, 49), "one_bin": (1, 24000, 24000), "ten_samples": (1000, 10, 1),
        "sr96000": (500, 48000, 97), "masks_32": (2700, 129600, 49), "masks_off": (2750, 132000, 49),
    }[shape]
    assert (nb, ns, spb) == expect
    if shape == "sr44100":
        assert ns % 16 == 4 and ns % BLOCK != 0 and nb * spb > ns
    if shape == "masks_32":
        assert 31 * BLOCK < ns <= 32 * BLOCK
    if shape == "masks_off":
        assert 32 * BLOCK < ns <= 33 * BLOCK
    if shape == "short_250ms":
        assert nb < 256 < 1000                                          # below the default LDS window
    if shape == "ten_samples":
        assert nb > ns


def test_restatement_agrees_with_the_loop_form(oracle_mod):
    """the vectorised reconstruct_f64 here equals the loop form of test_independent_restatement.py and the oracle"""
    from test_independent_restatement import reconstruct_f64 as loop_form
    rng = np.random.default_rng(8)
    for nb, ns, spb in ((1000, 48000, 49), (500, 22050, 45), (20, 960, 49), (1, 600, 600), (1000, 10, 1), (30, 1500, 7)):
        e = synthetic_energy(rng, 1, nb)[0]
        got = reconstruct_f64(e, ns, spb)
        want = loop_form(np.where(np.abs(e) >= np.float32(1e-6), e, 0.0), num_samples=ns, samples_per_bin=spb)
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-30)
        ref = oracle_mod.reconstruct(e, num_samples=ns, samples_per_bin=spb)
        assert np.abs(ref - got).max() <= 1e-6 * np.abs(got).max()
