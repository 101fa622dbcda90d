"""fs_reverb_set_soundfield: a diffuse late field on the ambisonic bus (include/frequensee.h and DESIGN.md section 8, "Soundfield
late reverb").

The carriers and the channel IRs are restated here in numpy (float64) from the definition in include/frequensee.h:
  channel c < C = (order + 1)^2, bin k in [1, K/2): seed_c = 0x5EED + (c << 32), phi_{c,k} = 2 pi (splitmix64(seed_c + k) >> 40) 2^-24;
  the spectrum of (c, band b) is exp(i phi_{c,k}) on the band's bins (cosine and sine rounded to float once), r_{c,b} its real
  inverse transform, car_{c,b} = r_{c,b} sqrt(N / sum r_{c,b}^2);
  h_c = (1/sqrt(B)) sum_b env_b car_{c,b} * w_l, w_l = 1 / sqrt(2 l + 1), l = floor(sqrt(c)).
Callbacks are checked against float64 convolutions of the downmix d = 0.5f (in_L + in_R) with the IRs COPIED FROM THE DEVICE, under
the partitioned engine's tolerance: |got - want| <= 2e-5 * max(max|want|, 1e-3) over the callback's block.  IRs formed through the
carrier passes are held to rel_rms <= 1e-6, the ears' and the spectral IR's bound.

Contexts are sized like test_reverb_ears.py's: sample_rate = ns, one second, octave edges under the context's own Nyquist."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_direct_paths import device_free_bytes
from test_reverb_crossfade import TOL, CrossfadeModel, close
from test_reverb_ears import edges_for, install_envelopes, refused
from test_reverb_partitioned import CROSSFADE_SCHEDULES, conv_f64, noise_blocks
from test_spectral_ir import band_of_bins, carriers, rel_rms, splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, PARTITIONED = 0, 1
SEED = 0x5EED
NEW = ["fs_reverb_soundfield_set", "fs_reverb_soundfield_info", "fs_reverb_set_soundfield",
       "fs_reverb_copy_soundfield_impulse_responses", "fs_reverb_soundfield_process_batch"]


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def channels(order):
    return (order + 1) ** 2


def degree(c):
    return int(np.floor(np.sqrt(c)))


def soundfield_carriers(C_, B, N, fs, edges=None):
    """car [C][B][N] float64, and the bin count n_b of every band"""
    band, K = band_of_bins(B, N, fs, edges)
    k = np.arange(K, dtype=np.uint64)
    car = np.empty((C_, B, N))
    for c in range(C_):
        seed = np.uint64(SEED + (c << 32))
        phi = 2.0 * np.pi * (splitmix64(seed + k) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
        X = np.cos(phi).astype(np.float32).astype(np.float64) + 1j * np.sin(phi).astype(np.float32).astype(np.float64)
        for b in range(B):
            r = (np.fft.ifft(np.where(band == b, X, 0.0)) * K).real[:N]
            car[c, b] = r * np.sqrt(N / np.sum(r * r))
    return car, np.array([int(np.sum(band == b)) for b in range(B)])


def soundfield_irs(env, car):
    """h [C][N] float64 of the band rows env [B][N]"""
    B = env.shape[0]
    e = env.astype(np.float64)
    return np.stack([np.sum(e * car[c], axis=0) / np.sqrt(B) / np.sqrt(2 * degree(c) + 1) for c in range(car.shape[0])])


_carriers = {}


def carriers_for(C_, B, ns, edges):
    """the largest set of a (B, ns, edges) is built once; a smaller order is its first channels"""
    key = (B, ns, None if edges is None else tuple(edges))
    if key not in _carriers or _carriers[key].shape[0] < C_:
        car, _ = soundfield_carriers(C_, B, ns, ns, edges)
        car.setflags(write=False)
        _carriers[key] = car
    return _carriers[key][:C_]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_exported_bound_and_listed(pkg):
    lib = pkg._capi.load()
    header = open(os.path.join(ROOT, "include", "frequensee.h")).read()
    head = header[:header.index("#ifndef")]
    ext = set(re.findall(r"fs_[a-z0-9_]+", head[head.index("EXTENDED:"):head.index("(tests/test_capi_cpu.py")]))
    for name in NEW:
        assert name in pkg._capi.EXPORTS and hasattr(lib, name) and name in ext, name
        assert getattr(lib, name).argtypes is not None
    for m in ("reverb_soundfield_set", "reverb_soundfield_info", "reverb_set_soundfield", "reverb_soundfield_impulse_responses",
              "reverb_soundfield_process_batch"):
        assert hasattr(pkg.Context, m), m
    assert issubclass(pkg.FrequenSeeAudioSoundfieldReverbPlugin, pkg.FrequenSeeAudioReverbPlugin)
    assert lib.fs_abi_version() == 5, "the change only adds"
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integration, name
    mirror = open(os.path.join(ROOT, "audio-pathtracer_amd", "host", "FrequenSee.hpp")).read()
    assert "class FrequenSeeAudioSoundfieldReverbPlugin : public FrequenSeeAudioReverbPlugin" in mirror


def test_null_context_is_an_invalid_argument(pkg):
    lib = pkg._capi.load()
    bad = pkg._capi.ERR_INVALID_ARGUMENT
    buf = np.zeros(8, np.float32)
    src = np.zeros(1, np.int32)
    assert lib.fs_reverb_soundfield_set(None, 1) == bad and lib.fs_reverb_soundfield_set(None, -1) == bad
    assert lib.fs_reverb_soundfield_info(None, None, None) == bad
    assert lib.fs_reverb_set_soundfield(None, 0, 1) == bad
    assert lib.fs_reverb_copy_soundfield_impulse_responses(None, 0, buf.ctypes.data, 4) == bad
    assert lib.fs_reverb_soundfield_process_batch(None, src.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, 0, None) == bad


def test_header_states_what_is_restated_here():
    header = open(os.path.join(ROOT, "include", "frequensee.h")).read()
    assert "seed_c = 0x5EED + (c << 32)" in header and "phi_{c,k} = 2 pi (splitmix64(seed_c + k) >> 40) 2^-24" in header
    assert "w_l = 1.0f / sqrtf((float)(2 l(c) + 1)), w_0 = 1.0f exactly" in header
    assert "m = m * (1.0f / sqrtf((float)B));" in header and "h_c[n] = m * w_l;" in header
    assert "G_{q,p} = FFT_N(h_{2q} + i h_{2q+1})" in header and "P = ceil(C / 2) pairs" in header
    assert "d(n) = 0.5f * (in[2n] + in[2n + 1])" in header
    assert "the ambisonic voices are late by (T - 1) / 2 samples and this reverb is not" in header
    assert "h_0 has the same bits as h_L of the two-ear reverb with an ear set of radius_cm = 0" in header
    assert "mono output to channel 0" not in header   # (the ambisonic renderer's text no longer sends hosts to the workaround)


@pytest.mark.parametrize("B,N", [(8, 48000), (8, 6000), (3, 6000), (1, 6000), (8, 4097), (8, 1000), (8, 12000)])
def test_restated_carriers_invariants(B, N):
    """unit mean power per (c, b); channel 0 is the spectral IR's carrier; any two channels of a band are as little correlated
    as independent noise of n_b bins: |corr| <= 4 / sqrt(n_b) (a condition on the seed rule, not a measurement)"""
    C_ = 16
    edges = edges_for(B, N)
    car, n_b = soundfield_carriers(C_, B, N, N, edges)
    assert np.allclose(np.mean(car * car, axis=2), 1.0, rtol=0, atol=1e-12)
    assert rel_rms(car[0], carriers(B, N, N, edges)) <= 1e-6
    worst = 0.0
    for b in range(B):
        m = car[:, b, :]
        corr = (m @ m.T) / np.sqrt(np.outer(np.sum(m * m, axis=1), np.sum(m * m, axis=1)))
        off = np.abs(corr - np.diag(np.diag(corr))).max()
        worst = max(worst, off * np.sqrt(n_b[b]))
        assert off <= 4.0 / np.sqrt(n_b[b]), (b, off, n_b[b])
    print(f"carriers B={B} N={N}: largest |corr| sqrt(n_b) over 120 pairs and {B} bands = {worst:.2f} (bound 4)")


# ---- GPU: helpers ---------------------------------------------------------------------------------------------------------------

#          ns     F   B  order
SHAPES = [(6000, 16, 1, 0), (6000, 16, 8, 1), (6000, 48, 3, 2), (6000, 48, 8, 3),
          (4097, 64, 8, 2), (1000, 1024, 8, 1), (12000, 2048, 8, 3), (48000, 1024, 8, 3)]


def make_ctx(pkg, ns, B, order, count=1, install=True):
    ctx = pkg.Context(num_bands=B, sample_rate=ns, simulated_duration=1.0)
    assert ctx.num_samples == ns
    edges = edges_for(B, ns)
    if edges is not None:
        ctx.set_band_edges(edges)
    if install:
        ctx.reverb_soundfield_set(order)
        assert ctx.reverb_soundfield_info() == (order, True)
    return ctx, [ctx.create_source((0.0, 0.0, 0.0)) for _ in range(count)], edges


def field_source(ctx, s, frame, fade=0):
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_set_ears(s, False)
    ctx.reverb_set_soundfield(s, True)
    if fade:
        ctx.reverb_set_crossfade(s, fade)
    ctx.reverb_init(s, frame)


def downmix(x):
    """[calls][2 F] float32 -> [calls][F] float32, the callback's own expression"""
    return np.float32(0.5) * (x[:, 0::2] + x[:, 1::2])


def expected_bus(x, h, frame):
    """[calls][F][C] float64: the downmix stream convolved with every channel's IR"""
    calls = x.shape[0]
    stream = downmix(x).astype(np.float64).reshape(-1)
    return np.stack([conv_f64(stream, np.asarray(hc, np.float64), stream.size).reshape(calls, frame) for hc in h], axis=2)


def one(ctx, s, blk):
    return ctx.reverb_soundfield_process_batch([s], blk[None])[0]


def check_stream(ctx, s, x, h, frame, what=""):
    y = np.stack([one(ctx, s, x[c]) for c in range(x.shape[0])])
    want = expected_bus(x, h, frame)
    worst = max(np.abs(y[c] - want[c]).max() / (TOL * max(np.abs(want[c]).max(), 1e-3)) for c in range(x.shape[0]))
    print(f"soundfield parity {what}: largest error = {worst:.4f} of the tolerance, peak |want| = {np.abs(want).max():.3f}")
    for c in range(x.shape[0]):
        assert close(y[c], want[c]), (what, c, np.abs(y[c] - want[c]).max())
    return y, want


# ---- GPU 1: the IRs against the restatement -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ns,frame,B,order", SHAPES)
def test_irs_against_the_restatement(pkg, ns, frame, B, order):
    C_ = channels(order)
    ctx, (s,), edges = make_ctx(pkg, ns, B, order)
    rng = np.random.default_rng(ns + frame + B)
    car = carriers_for(C_, B, ns, edges)

    def check(env, car, what):
        got, want = ctx.reverb_soundfield_impulse_responses(s), soundfield_irs(env, car)
        assert got.shape == (C_, ns)
        errs = [rel_rms(got[c], want[c]) for c in range(C_)]
        print(f"soundfield IRs ns={ns} B={B} order={order} {what}: largest rel rms {max(errs):.3e}")
        assert max(errs) <= 1e-6, (what, errs)
        if C_ > 1:   # two channels swapped must show
            assert rel_rms(got[1], want[2]) > 1e-2 and rel_rms(got[0], want[C_ - 1]) > 1e-2
        return got

    for flags in (0, 512):   # (whatever flags the reconstruct had)
        env = install_envelopes(pkg, ctx, s, rng, flags)
        check(env, car, f"flags={flags}")
    if B > 1:   # after fs_set_band_edges: the set moved
        base = edges if edges is not None else [125.0 * 2.0 ** (b - 0.5) for b in range(1, B)]
        moved = [float(np.float32(e * 0.8)) for e in base]
        before = ctx.reverb_soundfield_impulse_responses(s)
        ctx.set_band_edges(moved)
        assert ctx.reverb_soundfield_info() == (order, True)
        car, _ = soundfield_carriers(C_, B, ns, ns, moved)
        after = check(env, car, "moved edges")
        assert rel_rms(after[0], before[0]) > 1e-3
    ir = (rng.normal(0, 1, ns) * np.exp(-np.arange(ns) / (ns / 3.0)) * 0.004).astype(np.float32)
    ctx.set_impulse_response(s, ir)   # every band row is the installed IR
    check(np.tile(ir, (B, 1)), car, "installed IR")
    ctx.close()


# ---- GPU 2: W is the coherent ear -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ns,frame,B", [(6000, 48, 8), (48000, 1024, 8)])
def test_w_is_the_coherent_ear(pkg, ns, frame, B):
    ctx, (s,), _ = make_ctx(pkg, ns, B, 1)
    ctx.reverb_ears_set(radius_cm=0.0)
    install_envelopes(pkg, ctx, s, np.random.default_rng(ns))
    left, right = ctx.reverb_ear_impulse_responses(s)
    h = ctx.reverb_soundfield_impulse_responses(s)
    assert left.any() and h[0].tobytes() == left.tobytes() == right.tobytes()
    assert not np.array_equal(h[1], h[0])
    ctx.close()


# ---- GPU 3: the degree powers ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_degree_powers(pkg):
    """a constant energy in one band makes env_b constant, so h_c = env_b car_{c,b} w_l / sqrt(B) has the carrier's unit mean power
    times w_l^2: sum h_c^2 / sum h_0^2 = 1 / (2 l + 1)"""
    B = 4
    ctx = pkg.Context(num_bands=B)
    ctx.reverb_soundfield_set(3)
    s = ctx.create_source((0.0, 0.0, 0.0))
    for b in (1, 3):
        e = np.zeros((B, ctx.num_bins), np.float32)
        e[b] = 0.02
        ctx.update_energy_buffer(s, e)
        ctx.reconstruct_impulse_response(s, pkg.default_params())
        env = ctx.band_impulse_response(s, b)
        assert env.any()
        print(f"degree powers band {b}: env spread {np.ptp(env):.3e} of {env.max():.3e}")
        h = ctx.reverb_soundfield_impulse_responses(s).astype(np.float64)
        p = np.sum(h * h, axis=1)
        assert p[0] > 0
        for c in range(16):
            assert abs(p[c] / p[0] - 1.0 / (2 * degree(c) + 1)) <= 1e-5, (b, c, p[c] / p[0])
    ctx.close()


# ---- GPU 4: callback parity -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ns,frame,B,order", SHAPES)
def test_callback_parity(pkg, ns, frame, B, order):
    """independent noise in the two channels, K + 4 callbacks (the spectrum ring wraps); then, from a released state, in_R = -in_L:
    the downmix is zero and every channel is silent to the bit; then a block loud enough for |W| > 1: it comes back unclamped"""
    K = -(-ns // frame)
    ctx, (s,), _ = make_ctx(pkg, ns, B, order)
    rng = np.random.default_rng(7 * ns + frame + B)
    install_envelopes(pkg, ctx, s, rng)
    h = ctx.reverb_soundfield_impulse_responses(s)
    field_source(ctx, s, frame)
    x = noise_blocks(rng, K + 4, frame)
    y, want = check_stream(ctx, s, x, h, frame, what=f"ns={ns} F={frame} B={B} order={order}")
    assert y.shape == (K + 4, frame, channels(order)) and np.abs(want).max() > 0.02
    ctx.reverb_release(s)
    x = noise_blocks(rng, 3, frame)
    x[:, 1::2] = -x[:, 0::2]
    for c in range(3):
        assert not one(ctx, s, x[c]).any(), c
    ctx.reverb_release(s)
    x = noise_blocks(rng, min(K + 1, 6), frame)
    quiet = np.abs(expected_bus(x, h[:1], frame)).max()
    x = x * np.float32(2.0 ** np.ceil(np.log2(1.5 / quiet)))   # (a power of two: the scaled stream is exact)
    y, want = check_stream(ctx, s, x, h, frame, what=f"ns={ns} F={frame} B={B} order={order} loud")
    assert np.abs(want[:, :, 0]).max() > 1.0 and np.abs(y[:, :, 0]).max() > 1.0
    ctx.close()


# ---- GPU 5: crossfade -----------------------------------------------------------------------------------------------------------

NS_X, F_X, B_X, ORDER_X = 6000, 64, 3, 2


class FieldModel:
    """CrossfadeModel per channel, fed the downmix in both of its inputs: its left output is the channel.  (Its +-1 clamp is never
    reached at these levels.)"""

    def __init__(self, n, frame, fade_len, C_):
        self.m = [CrossfadeModel(n, frame, fade_len) for _ in range(C_)]

    def install(self, h):
        for m, hc in zip(self.m, h):
            m.install(hc)

    def set_crossfade(self, L):
        for m in self.m:
            m.set_crossfade(L)

    def release(self):
        for m in self.m:
            m.release()

    def process(self, blk):
        d = downmix(blk[None])[0]
        both = np.repeat(d, 2)
        out = np.stack([m.process(both)[0::2] for m in self.m], axis=1)
        assert np.abs(out).max() < 1.0
        return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CROSSFADE_SCHEDULES))
def test_crossfade_rules_per_channel(pkg, name):
    """test_reverb_partitioned.py's schedules at order 2 (C = 9: the last pair has no partner).  'literal' and 'bypass' name
    what this call does not have: those callbacks are plain ones."""
    L, schedule = CROSSFADE_SCHEDULES[name]
    C_ = channels(ORDER_X)
    ctx, (s,), _ = make_ctx(pkg, NS_X, B_X, ORDER_X)
    field_source(ctx, s, F_X, fade=L)
    model = FieldModel(NS_X, F_X, L, C_)
    rng = np.random.default_rng(len(name))
    for step, actions in enumerate(schedule):
        for act in actions:
            if act == "ir":
                install_envelopes(pkg, ctx, s, rng)
                model.install(ctx.reverb_soundfield_impulse_responses(s))
            elif act == "release":
                ctx.reverb_release(s)
                model.release()
            elif act in ("literal", "bypass"):
                pass
            else:
                ctx.reverb_set_crossfade(s, act[1])
                model.set_crossfade(act[1])
        blk = noise_blocks(rng, 1, F_X)[0]
        got, want = one(ctx, s, blk), model.process(blk)
        assert close(got, want), (step, actions, np.abs(got - want).max())
    ctx.close()


@pytest.mark.gpu
def test_replacing_the_set_goes_through_the_crossfade(pkg):
    """fs_set_band_edges rebuilds the set and bumps its generation: the source takes again at its next callback, fading from
    the tuple it heard"""
    L = 200
    C_ = channels(ORDER_X)
    ctx, (s,), edges = make_ctx(pkg, NS_X, B_X, ORDER_X)
    rng = np.random.default_rng(5)
    install_envelopes(pkg, ctx, s, rng)
    field_source(ctx, s, F_X, fade=L)
    model, abrupt = FieldModel(NS_X, F_X, L, C_), FieldModel(NS_X, F_X, 0, C_)
    for m in (model, abrupt):
        m.install(ctx.reverb_soundfield_impulse_responses(s))
    for c, blk in enumerate(noise_blocks(rng, 10, F_X)):
        if c == 3:
            before = ctx.reverb_soundfield_impulse_responses(s)
            ctx.set_band_edges([float(np.float32(e * 0.8)) for e in edges])
            h = ctx.reverb_soundfield_impulse_responses(s)
            assert not np.array_equal(h, before)
            for m in (model, abrupt):
                m.install(h)
        got, want, switched = one(ctx, s, blk), model.process(blk), abrupt.process(blk)
        assert close(got, want), (c, np.abs(got - want).max())
        if c == 3:
            assert not close(got, switched), "the fade is heard: an abrupt switch is another signal"
    ctx.close()


# ---- GPU 6: batching ------------------------------------------------------------------------------------------------------------

CALLS_B = 8


def drive(pkg, n, serve, order=ORDER_X, stereo=None, field=True):
    """n soundfield sources driven alike whatever serves them: source 0 fades, IRs change on the way.  stereo(ctx, c): a stereo
    callback of other sources in the same context before soundfield callback c; field == False: the context never sees a soundfield"""
    ctx, srcs, _ = make_ctx(pkg, NS_X, B_X, order, count=n + 3, install=field)
    srcs, others = srcs[:n], srcs[n:]
    rng = np.random.default_rng(66)
    for s in srcs + others:
        install_envelopes(pkg, ctx, s, rng)
    if field:
        for i, s in enumerate(srcs):
            field_source(ctx, s, F_X, fade=200 if i == 0 else 0)
    if stereo is not None:
        ctx.reverb_ears_set(radius_cm=8.75 * 48000.0 / NS_X)
        for s, kind in zip(others, ("part", "ear", "direct")):
            ctx.reverb_set_engine(s, DIRECT if kind == "direct" else PARTITIONED)
            ctx.reverb_set_ears(s, kind == "ear")
            ctx.reverb_init(s, F_X)
    res, side = [], []
    for c in range(CALLS_B):
        if c in (2, 3, 6):
            install_envelopes(pkg, ctx, srcs[0], rng)
        if c == 5:
            install_envelopes(pkg, ctx, srcs[-1], rng)
            install_envelopes(pkg, ctx, others[0], rng)
        blk = noise_blocks(rng, n, F_X)
        other_blk = noise_blocks(rng, 3, F_X)
        if stereo is not None:
            side.append(ctx.reverb_process_batch(others, other_blk, want_out=True, want_mix=True))
        if field:
            res.append(serve(ctx, srcs, blk))
    ctx.close()
    return res, side


def serve_single(ctx, srcs, blk):
    return np.stack([one(ctx, s, blk[i]) for i, s in enumerate(srcs)])


def serve_batch(ctx, srcs, blk):
    return ctx.reverb_soundfield_process_batch(srcs, blk, want_out=True, want_mix=True)


def serve_permuted(ctx, srcs, blk):
    perm = [2, 0, 3, 1]
    out = ctx.reverb_soundfield_process_batch([srcs[i] for i in perm], blk[perm])
    back = np.empty_like(out)
    back[perm] = out
    return back


def serve_three_modes(ctx, srcs, blk):
    """alternating return modes; what a mode leaves out is None"""
    serve_three_modes.calls += 1
    mode = serve_three_modes.calls % 3
    if mode == 0:
        return ctx.reverb_soundfield_process_batch(srcs, blk, want_out=True, want_mix=True)
    if mode == 1:
        return ctx.reverb_soundfield_process_batch(srcs, blk, want_out=True, want_mix=False), None
    return None, ctx.reverb_soundfield_process_batch(srcs, blk, want_out=False, want_mix=True)


@pytest.mark.gpu
def test_one_call_or_several_or_permuted_to_the_bit(pkg):
    single, _ = drive(pkg, 4, serve_single)
    both, _ = drive(pkg, 4, serve_batch)
    permuted, _ = drive(pkg, 4, serve_permuted)
    serve_three_modes.calls = 0
    modes, _ = drive(pkg, 4, serve_three_modes)
    assert max(np.abs(o).max() for o in single) > 0.02
    for c in range(CALLS_B):
        out, mix = both[c]
        assert out.tobytes() == single[c].tobytes() == permuted[c].tobytes(), c
        want = out[0].copy()
        for r in range(1, 4):
            want = want + out[r]   # fp32, list order
        assert mix.tobytes() == want.tobytes(), c
        o, m = modes[c]
        assert o is None or o.tobytes() == out.tobytes(), c
        assert m is None or m.tobytes() == mix.tobytes(), c
        assert not np.array_equal(out[0][:, 0], out[0][:, 1])


@pytest.mark.gpu
def test_stereo_rows_keep_their_bits(pkg):
    """a stereo batch of a partitioned, an ear and a direct row between soundfield callbacks gives the bits of a context that never
    saw a soundfield"""
    _, with_field = drive(pkg, 4, serve_batch, stereo=True)
    _, without = drive(pkg, 4, serve_batch, stereo=True, field=False)
    assert len(with_field) == len(without) == CALLS_B
    for c in range(CALLS_B):
        assert with_field[c][0].tobytes() == without[c][0].tobytes() and with_field[c][1].tobytes() == without[c][1].tobytes(), c
    assert max(np.abs(o[0]).max() for o in without) > 0.02


# ---- GPU 7: steady state --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    n = 12
    ctx, srcs, _ = make_ctx(pkg, NS_X, B_X, 3, count=n)
    rng = np.random.default_rng(40)
    for i, s in enumerate(srcs):
        install_envelopes(pkg, ctx, s, rng)
        field_source(ctx, s, F_X, fade=100 if i % 2 else 0)
    blk = noise_blocks(rng, n, F_X)
    ctx.reverb_soundfield_process_batch(srcs, blk, want_out=True, want_mix=True)
    free0 = device_free_bytes()
    for cb in range(12):
        if cb % 3 == 0:
            install_envelopes(pkg, ctx, srcs[cb % n], rng)   # takes and fades on the way
        ctx.reverb_soundfield_process_batch(srcs, blk, want_out=bool(cb % 2), want_mix=True)
    ctx.reverb_soundfield_process_batch(srcs[:5], blk[:5])   # a smaller shape fits what is there
    assert device_free_bytes() >= free0
    ctx.close()


# ---- GPU 8: refusals change nothing ---------------------------------------------------------------------------------------------

def refusal_run(pkg, disturb):
    """a soundfield source's callbacks with disturb(ctx, s, other, third) between them (None: the undisturbed run); `other` is a
    plain partitioned source of the same frame size, `third` has no reverb yet"""
    ctx, (s, other, third), _ = make_ctx(pkg, NS_X, B_X, 1, count=3)
    rng = np.random.default_rng(21)
    install_envelopes(pkg, ctx, s, rng)
    field_source(ctx, s, F_X)
    ctx.reverb_set_engine(other, PARTITIONED)
    ctx.reverb_init(other, F_X)
    x = noise_blocks(rng, 6, F_X)
    out = []
    for c in range(6):
        if c in (2, 4) and disturb is not None:
            disturb(ctx, s, other, third)
            assert ctx.reverb_soundfield_info() == (1, True)
        out.append(one(ctx, s, x[c]))
    ctx.close()
    return np.stack(out)


_undisturbed = {}


def undisturbed(pkg):
    if "out" not in _undisturbed:
        out = refusal_run(pkg, None)
        assert np.abs(out).max() > 0.02
        out.setflags(write=False)
        _undisturbed["out"] = out
    return _undisturbed["out"]


def raw_batch(ctx, handles, frame, C_, flags=0, out=True, mix=False):
    srcs = np.asarray(handles, np.int32)
    blk = np.zeros((len(handles), 2 * frame), np.float32)
    o = np.zeros((len(handles), frame * C_), np.float32)
    m = np.zeros(frame * C_, np.float32)
    ctx.check(ctx.lib.fs_reverb_soundfield_process_batch(ctx.h, srcs.ctypes.data, len(handles), blk.ctypes.data,
                                                         o.ctypes.data if out else None, flags, m.ctypes.data if mix else None))


def init_other_frame(ctx, third):
    field_source(ctx, third, 2 * F_X)


REFUSALS = {
    "init_with_ears_as_well":
        lambda pkg, ctx, s, o, t: (ctx.reverb_ears_set(radius_cm=10.0), ctx.reverb_set_engine(t, PARTITIONED), ctx.reverb_set_ears(t, True),
                                   ctx.reverb_set_soundfield(t, True),
                                   refused(pkg, ctx, lambda: ctx.reverb_init(t, F_X), "fs_reverb_set_soundfield", "fs_reverb_set_ears")),
    "init_under_the_direct_engine":
        lambda pkg, ctx, s, o, t: (ctx.reverb_set_engine(t, DIRECT), ctx.reverb_set_soundfield(t, True),
                                   refused(pkg, ctx, lambda: ctx.reverb_init(t, F_X), "FS_REVERB_ENGINE_PARTITIONED")),
    "flags_not_zero":
        lambda pkg, ctx, s, o, t: refused(pkg, ctx, lambda: raw_batch(ctx, [s], F_X, 4, flags=1), "flags must be 0"),
    "a_duplicate_handle":
        lambda pkg, ctx, s, o, t: refused(pkg, ctx, lambda: raw_batch(ctx, [s, s], F_X, 4), "twice"),
    "mixed_frame_sizes":
        lambda pkg, ctx, s, o, t: (init_other_frame(ctx, t), refused(pkg, ctx, lambda: raw_batch(ctx, [s, t], F_X, 4), "one frame size")),
    "a_source_without_the_soundfield":
        lambda pkg, ctx, s, o, t: refused(pkg, ctx, lambda: raw_batch(ctx, [s, o], F_X, 4), "not initialised with the soundfield"),
    "a_soundfield_source_in_the_stereo_batch":
        lambda pkg, ctx, s, o, t: refused(pkg, ctx, lambda: ctx.reverb_process_batch([o, s], np.zeros((2, 2 * F_X), np.float32)),
                                          "fs_reverb_soundfield_process_batch"),
    "a_soundfield_source_in_the_stereo_call":
        lambda pkg, ctx, s, o, t: (refused(pkg, ctx, lambda: ctx.reverb_process(s, np.zeros(2 * F_X, np.float32)), "fs_reverb_soundfield_process_batch"),
                                   refused(pkg, ctx, lambda: ctx.reverb_process(s, np.zeros(2 * F_X, np.float32), apply_reverb=False),
                                           "fs_reverb_soundfield_process_batch")),
    "clearing_the_set":
        lambda pkg, ctx, s, o, t: refused(pkg, ctx, lambda: ctx.reverb_soundfield_set(clear=True), "initialised with the soundfield"),
    "changing_the_order":
        lambda pkg, ctx, s, o, t: (refused(pkg, ctx, lambda: ctx.reverb_soundfield_set(2), "initialised with the soundfield"),
                                   ctx.reverb_soundfield_set(1)),   # (the order installed: FS_OK, nothing changes)
    "order_4":
        lambda pkg, ctx, s, o, t: refused(pkg, ctx, lambda: ctx.reverb_soundfield_set(4), "FS_MAX_AMBISONIC_ORDER"),
    "a_band_without_a_bin":
        lambda pkg, ctx, s, o, t: refused(pkg, ctx, lambda: ctx.set_band_edges([100.0, 100.1]), "fs_set_band_edges", "at least one FFT bin"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_change_nothing(pkg, name):
    got = refusal_run(pkg, lambda ctx, s, o, t: REFUSALS[name](pkg, ctx, s, o, t))
    assert got.tobytes() == undisturbed(pkg).tobytes(), name


@pytest.mark.gpu
def test_out_and_mix_both_null(pkg):
    def disturb(ctx, s, o, t):
        srcs = np.asarray([s], np.int32)
        blk = np.zeros((1, 2 * F_X), np.float32)
        rc = ctx.lib.fs_reverb_soundfield_process_batch(ctx.h, srcs.ctypes.data, 1, blk.ctypes.data, None, 0, None)
        assert rc == pkg._capi.ERR_INVALID_ARGUMENT
    assert refusal_run(pkg, disturb).tobytes() == undisturbed(pkg).tobytes()


@pytest.mark.gpu
def test_refusals_without_a_set(pkg):
    """the soundfield on with no set installed; the copy without a set; a set whose band edges leave a band without a bin — then
    the good calls, and the callbacks of the undisturbed run"""
    ctx, (s, other, third), _ = make_ctx(pkg, NS_X, B_X, 1, count=3, install=False)
    assert ctx.reverb_soundfield_info() == (-1, False)
    ctx.reverb_soundfield_set(clear=True)                # nothing to clear: fine
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_set_soundfield(s, True)
    refused(pkg, ctx, lambda: ctx.reverb_init(s, F_X), "no soundfield set is installed")
    refused(pkg, ctx, lambda: ctx.reverb_soundfield_impulse_responses(s), "no soundfield set is installed")
    ctx2 = pkg.Context(num_bands=8, sample_rate=NS_X, simulated_duration=1.0)   # (the default octave edges at 6 kHz)
    refused(pkg, ctx2, lambda: ctx2.reverb_soundfield_set(1), "fs_reverb_soundfield_set", "at least one FFT bin")
    assert ctx2.reverb_soundfield_info() == (-1, False)
    ctx2.close()
    ctx.reverb_soundfield_set(1)
    rng = np.random.default_rng(21)
    install_envelopes(pkg, ctx, s, rng)
    ctx.reverb_init(s, F_X)                              # (the recorded choices held through the refusals)
    x = noise_blocks(rng, 6, F_X)
    got = np.stack([one(ctx, s, x[c]) for c in range(6)])
    assert got.tobytes() == undisturbed(pkg).tobytes()
    ctx.reverb_set_soundfield(s, False)                  # without the soundfield again: the set can change and go
    ctx.reverb_init(s, F_X)
    ctx.reverb_soundfield_set(3)
    assert ctx.reverb_soundfield_info() == (3, True)
    ctx.reverb_soundfield_set(clear=True)
    assert ctx.reverb_soundfield_info() == (-1, False)
    ctx.close()


# ---- GPU 9: the layers above ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_plugin_against_the_c_call(pkg):
    frame, order = 256, 2
    rng = np.random.default_rng(3)
    ir = (rng.normal(0, 1, 48000) * np.exp(-np.arange(48000) / 4000.0) * 0.02).astype(np.float32)
    x = noise_blocks(rng, 3, frame)

    def world():
        sub = pkg.AudioRayTracingSubsystem(num_bands=2, device=0)
        comps = [pkg.FrequenSeeAudioComponent((0.0, 0.0, 0.0)) for _ in range(2)]
        for c in comps:
            c.OnRegister(sub)
            sub.ctx.set_impulse_response(c._src, ir)
        return sub, comps

    sub, comps = world()
    plug = pkg.FrequenSeeAudioSoundfieldReverbPlugin(sub)
    plug.Initialize(frame)
    plug.SetOrder(order)
    for c in comps:
        c.bApplyReverb = False   # (not read: the call has no bypass row)
        plug.OnInitSource(c)
    sub2, comps2 = world()
    sub2.ctx.reverb_soundfield_set(order)
    for c in comps2:
        field_source(sub2.ctx, c._src, frame)
    assert np.array_equal(plug.ImpulseResponses(comps[0]), sub2.ctx.reverb_soundfield_impulse_responses(comps2[0]._src))
    for cb in range(3):
        blk = np.stack([x[cb], x[(cb + 1) % 3]])
        got, gmix = plug.ProcessAudio(comps, blk, want_mix=True)
        want, wmix = sub2.ctx.reverb_soundfield_process_batch([c._src for c in comps2], blk, want_out=True, want_mix=True)
        assert got.shape == (2, frame, channels(order)) and got.any()
        assert got.tobytes() == want.tobytes() and gmix.tobytes() == wmix.tobytes()
    assert plug.ProcessSourceAudio(comps[0], x[0]).shape == (frame, channels(order))
    sub.Deinitialize()
    sub2.Deinitialize()


@pytest.mark.gpu
def test_cpp_mirror_plugin(pkg, tmp_path):
    """host/FrequenSee.hpp's FrequenSeeAudioSoundfieldReverbPlugin through the headless harness: SetOrder(1), OnInitSource, one
    callback of a half-scale unit impulse and ImpulseResponses — channel c of the block is 0.5 h_c within the engine's tolerance,
    which is what the Python plugin gives for the same block (test_plugin_against_the_c_call holds it to the C call)"""
    exe = os.path.join(os.path.dirname(pkg._capi.LIB_PATH), "fs_harness")
    r = subprocess.run([exe, "1", "256", "2", str(tmp_path / "ir.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert j["soundfield_peak"] > 0.01 and j["soundfield_channel_max_diff"] > 1e-3, j
    assert j["soundfield_max_err"] <= TOL * max(j["soundfield_peak"], 1e-3), j


@pytest.mark.gpu
def test_traced_room_in_one_bus(pkg, scene_factory):
    """a shoebox traced at min_order = 2 (the late part: the early paths are the voices'), order 1: the soundfield reverb's mix and
    the ambisonic renderer's mix of one direct voice summed into one bus — finite, and its late W is the convolution with h_0"""
    frame, order, taps = 1024, 1, 15
    sc = scene_factory("shoebox", 4)
    ctx = pkg.Context(num_bands=4)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    ctx.reverb_soundfield_set(order)
    s = ctx.create_source(sc.source)
    ctx.set_source_order_window(s, min_order=2)
    ctx.update_sources([s], pkg.default_params(num_rays=4096, depth=8, seed=300))   # (the reference's distance scale)
    h = ctx.reverb_soundfield_impulse_responses(s)
    assert h[0].any()
    field_source(ctx, s, frame)
    v = ctx.create_source(sc.source)   # the voices' source
    ctx.ambisonic_render_init(v, frame, taps, 4, 0.05, order)
    rng = np.random.default_rng(12)
    x = noise_blocks(rng, 6, frame)
    voice = [(1, 0.01, np.ones(8, np.float32), 0.5, (1.0, 0.5, 0.0))]
    late = []
    for c in range(6):
        early = ctx.ambisonic_render_process_batch([v], x[c][None], [voice], want_out=False, want_mix=True)[0]
        tail = ctx.reverb_soundfield_process_batch([s], x[c][None], want_out=False, want_mix=True)
        bus = early + tail
        assert bus.shape == (frame, channels(order)) and np.isfinite(bus).all() and early.any()
        late.append(tail)
    want = expected_bus(x, h[:1], frame)
    assert np.abs(want).max() > 0
    for c in range(6):
        assert close(late[c][:, 0], want[c][:, 0]), (c, np.abs(late[c][:, 0] - want[c][:, 0]).max())
    ctx.close()
