"""fs_reverb_set_ears: a two-ear late field with the interaural coherence of a diffuse field (include/frequensee.h and DESIGN.md
section 8, "Two-ear late reverb").

The ear carriers and the ear IRs are restated here in numpy (float64) from the definition in include/frequensee.h:
  bin k in [1, K/2): f_k = k fs / K, x_k = 2 pi f_k (2 radius) / c, gamma_k = sin(x_k) / x_k, a_k = sqrt((1 + gamma_k) / 2),
  b_k = sqrt((1 - gamma_k) / 2); mid spectrum a_k exp(i phi_k), side spectrum b_k exp(i psi_k) (each product rounded to float
  once), r^M_b / r^S_b their real inverse transforms, one scale g_b = sqrt(N / sum (r^M_b^2 + r^S_b^2)) for both;
  m = (1/sqrt(B)) sum_b env_b cm_b, s likewise with cs_b; h_L = m + s, h_R = m - s.
Callbacks are checked against float64 convolutions with the ear IRs COPIED FROM THE DEVICE, under the partitioned engine's
tolerance: |got - want| <= 2e-5 * max(max|want|, 1e-3) over the callback's block.

Contexts are sized like test_reverb_partitioned.py's: sample_rate = ns, one second.  The default octave edges do not fit such
a rate, so those contexts get octave edges below their own Nyquist, and a head radius scaled by 48000 / ns: the same x_k per
bin index as the default head at 48 kHz, so the side term is as large as it is there."""
import copy
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from test_reverb_crossfade import TOL, CrossfadeModel, close, traced_params
from test_reverb_partitioned import CROSSFADE_SCHEDULES, conv_f64, noise_blocks
from test_spectral_ir import band_of_bins, rel_rms, splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, PARTITIONED = 0, 1
SEED_MID, SEED_SIDE = 0x5EED, 0x5EED0EA2
RADIUS, SPEED = 8.75, 34300.0            # FS_HRTF_DEFAULT_RADIUS_CM, FS_HRTF_DEFAULT_SOUND_SPEED_CM_S
NEW = ["fs_reverb_ears_default", "fs_reverb_ears_set", "fs_reverb_ears_info", "fs_reverb_set_ears",
       "fs_reverb_copy_ear_impulse_responses"]


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def gamma_of(K, fs, radius_cm, speed_cm_s):
    f = np.arange(K, dtype=np.float64) * float(fs) / float(K)
    x = 2.0 * np.pi * f * (2.0 * float(np.float32(radius_cm))) / float(np.float32(speed_cm_s))
    return np.where(x == 0.0, 1.0, np.sin(x) / np.where(x == 0.0, 1.0, x))


def ear_carriers(B, N, fs, radius_cm=RADIUS, speed_cm_s=SPEED, edges=None):
    """(cm, cs): [B][N] float64 each"""
    band, K = band_of_bins(B, N, fs, edges)
    k = np.arange(K, dtype=np.uint64)
    g = gamma_of(K, fs, radius_cm, speed_cm_s)
    a, b = np.sqrt((1.0 + g) / 2.0), np.sqrt(np.maximum(1.0 - g, 0.0) / 2.0)
    phi = 2.0 * np.pi * (splitmix64(np.uint64(SEED_MID) + k) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    psi = 2.0 * np.pi * (splitmix64(np.uint64(SEED_SIDE) + k) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24

    def once(w, ph):   # each product formed in double and rounded to float once
        return (w * np.cos(ph)).astype(np.float32).astype(np.float64) + 1j * (w * np.sin(ph)).astype(np.float32).astype(np.float64)

    XM, XS = once(a, phi), once(b, psi)
    cm, cs = np.empty((B, N)), np.empty((B, N))
    for q in range(B):
        rm = (np.fft.ifft(np.where(band == q, XM, 0.0)) * K).real[:N]
        rs = (np.fft.ifft(np.where(band == q, XS, 0.0)) * K).real[:N]
        scale = np.sqrt(N / np.sum(rm * rm + rs * rs))
        cm[q], cs[q] = scale * rm, scale * rs
    return cm, cs


def ear_irs(env, cm, cs):
    B = env.shape[0]
    e = env.astype(np.float64)
    m, s = np.sum(e * cm, axis=0) / np.sqrt(B), np.sum(e * cs, axis=0) / np.sqrt(B)
    return m + s, m - s


_carriers = {}


def carriers_for(B, ns, radius, edges):
    key = (B, ns, float(radius), None if edges is None else tuple(edges))
    if key not in _carriers:
        cm, cs = ear_carriers(B, ns, ns, radius, SPEED, edges)
        cm.setflags(write=False); cs.setflags(write=False)
        _carriers[key] = (cm, cs)
    return _carriers[key]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_exported_bound_and_listed(pkg):
    lib = pkg._capi.load()
    header = open(os.path.join(ROOT, "include", "frequensee.h")).read()
    head = header[:header.index("#ifndef")]
    ext = set(re.findall(r"fs_[a-z0-9_]+", head[head.index("EXTENDED:"):head.index("(tests/test_capi_cpu.py")]))
    for name in NEW:
        assert name in pkg._capi.EXPORTS and hasattr(lib, name) and name in ext, name
        assert getattr(lib, name).argtypes is not None
    for m in ("reverb_ears_set", "reverb_ears_info", "reverb_set_ears", "reverb_ear_impulse_responses"):
        assert hasattr(pkg.Context, m), m
    d = pkg._capi.default_reverb_ears()
    assert d.struct_size == C.sizeof(pkg._capi.ReverbEarsDesc) == 12
    assert (d.radius_cm, d.sound_speed_cm_s) == (np.float32(RADIUS), np.float32(SPEED))
    assert (pkg._capi.HRTF_DEFAULT_RADIUS_CM, pkg._capi.HRTF_DEFAULT_SOUND_SPEED_CM_S) == (RADIUS, SPEED)
    assert lib.fs_abi_version() == 5, "the change only adds"
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integration, name


def test_null_context_is_an_invalid_argument(pkg):
    lib = pkg._capi.load()
    bad = pkg._capi.ERR_INVALID_ARGUMENT
    d = pkg._capi.default_reverb_ears()
    buf = np.zeros(4, np.float32)
    assert lib.fs_reverb_ears_set(None, C.byref(d)) == bad and lib.fs_reverb_ears_set(None, None) == bad
    assert lib.fs_reverb_ears_info(None, None, None, None) == bad
    assert lib.fs_reverb_set_ears(None, 0, 1) == bad
    assert lib.fs_reverb_copy_ear_impulse_responses(None, 0, buf.ctypes.data, buf.ctypes.data, 4) == bad
    lib.fs_reverb_ears_default(None)   # (nothing to fill: no crash)


def test_header_states_what_is_restated_here():
    header = open(os.path.join(ROOT, "include", "frequensee.h")).read()
    assert "splitmix64(0x5EED + k) >> 40) 2^-24" in header and "splitmix64(0x5EED0EA2 + k) >> 40) 2^-24" in header
    assert "x_k = 2 pi f_k (2 radius_cm) / sound_speed_cm_s" in header and "gamma_k = sin(x_k) / x_k" in header
    assert "a_k = sqrt((1 + gamma_k) / 2)" in header and "b_k = sqrt((1 - gamma_k) / 2)" in header
    assert "h_L = m + s, h_R = m - s" in header


def test_restated_carriers_invariants():
    B, N, fs = 8, 48000, 48000
    cm, cs = ear_carriers(B, N, fs)
    L, R = cm + cs, cm - cs
    assert np.allclose(np.mean((L * L + R * R) / 2.0, axis=1), 1.0, rtol=0, atol=1e-12)
    band, K = band_of_bins(B, N, fs)
    g = gamma_of(K, fs, RADIUS, SPEED)
    for b in range(B):
        corr = np.sum(L[b] * R[b]) / np.sqrt(np.sum(L[b] ** 2) * np.sum(R[b] ** 2))
        assert abs(corr - g[band == b].mean()) <= 0.05, (b, corr, g[band == b].mean())
    cm0, cs0 = ear_carriers(B, N, fs, radius_cm=0.0)
    assert not cs0.any() and np.allclose(np.mean(cm0 * cm0, axis=1), 1.0, rtol=0, atol=1e-12)


# ---- GPU: helpers ---------------------------------------------------------------------------------------------------------------

SHAPES = [(6000, 48, 1), (6000, 48, 3), (6000, 48, 8), (6000, 16, 1), (6000, 16, 3), (6000, 16, 8),
          (4097, 64, 8), (1000, 1024, 8), (12000, 2048, 8), (48000, 1024, 8)]


def edges_for(B, ns):
    """None at 48 kHz (the default octave edges); else octave edges under the context's own Nyquist"""
    if ns == 48000 or B == 1:
        return None
    return [float(np.float32(0.45 * ns * 2.0 ** -(B - 1 - i))) for i in range(B - 1)]


def radius_for(ns):
    return float(np.float32(RADIUS * 48000.0 / ns))


def make_ctx(pkg, ns, B, count=1, radius=None, ears=True):
    ctx = pkg.Context(num_bands=B, sample_rate=ns, simulated_duration=1.0)
    assert ctx.num_samples == ns
    edges = edges_for(B, ns)
    if edges is not None:
        ctx.set_band_edges(edges)
    radius = radius_for(ns) if radius is None else radius
    if ears:
        ctx.reverb_ears_set(radius_cm=radius)
    return ctx, [ctx.create_source((0.0, 0.0, 0.0)) for _ in range(count)], edges, radius


def ear_source(ctx, s, frame, fade=0):
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_set_ears(s, True)
    if fade:
        ctx.reverb_set_crossfade(s, fade)
    ctx.reverb_init(s, frame)


def install_envelopes(pkg, ctx, s, rng, flags=0):
    """a decaying energy, every band different, a few zero blocks -> the device band rows [B][ns] (float32).  The level keeps
    the convolution of 0.3-rms noise around 0.1: 2.8 / ns at the first bin, a decay of nb / (2 + b) bins."""
    B, nb, ns = ctx.num_bands, ctx.num_bins, ctx.num_samples
    i = np.arange(nb, dtype=np.float64)
    e = np.array([(2.8 / ns) * np.exp(-i * (2 + b) / nb) * rng.uniform(0.5, 1.5, nb) for b in range(B)])
    e[:, 3:5] = 0.0
    e[:, nb // 2:nb // 2 + 3] = 0.0
    ctx.update_energy_buffer(s, e.astype(np.float32))
    ctx.reconstruct_impulse_response(s, pkg.default_params(flags=flags))
    env = np.array([ctx.band_impulse_response(s, b) for b in range(B)])
    assert env.any() and all(env[b].any() for b in range(B))
    return env


def expected_ears(x, h_left, h_right, frame, literal_odd):
    """[calls][2 * frame] float64: each channel's whole stream convolved with its ear's IR; literal_odd: odd callbacks with
    FS_REVERB_LITERAL_TAIL (the current block is the interleaved buffer's first `frame` floats in both channels)"""
    calls = x.shape[0]
    want = np.empty((calls, 2 * frame))
    for ch, h in enumerate((np.asarray(h_left, np.float64), np.asarray(h_right, np.float64))):
        stream = x[:, ch::2].astype(np.float64).reshape(-1)
        w = conv_f64(stream, h, stream.size).reshape(calls, frame)
        if literal_odd:
            for c in range(1, calls, 2):
                d = x[c, :frame].astype(np.float64) - x[c, ch::2].astype(np.float64)
                w[c] += conv_f64(d, h[:frame], frame)
        want[:, ch::2] = w
    return np.clip(want, -1.0, 1.0)


def check_stream(ctx, s, x, h_left, h_right, frame, literal_odd=False, what=""):
    y = np.stack([ctx.reverb_process(s, x[c], literal_tail=literal_odd and bool(c % 2)) for c in range(x.shape[0])])
    want = expected_ears(x, h_left, h_right, frame, literal_odd)
    worst = max(np.abs(y[c] - want[c]).max() / (TOL * max(np.abs(want[c]).max(), 1e-3)) for c in range(x.shape[0]))
    print(f"ears parity {what}: largest error = {worst:.4f} of the tolerance, peak |want| = {np.abs(want).max():.3f}")
    for c in range(x.shape[0]):
        assert close(y[c], want[c]), (what, c, np.abs(y[c] - want[c]).max())
    return y, want


# ---- GPU 1: the ear IRs against the restatement -----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ns,frame,B", SHAPES)
def test_ear_irs_against_the_restatement(pkg, ns, frame, B):
    """rel_rms <= 1e-6 per ear: the bound test_spectral_ir.py::test_exact_restatement_on_traced_frames holds the spectral row to,
    which runs through the same inverse passes and the same product"""
    ctx, (s,), edges, radius = make_ctx(pkg, ns, B)
    assert ctx.reverb_ears_info() == (radius, SPEED, True)
    rng = np.random.default_rng(ns + frame + B)
    cm, cs = carriers_for(B, ns, radius, edges)
    for flags in (0, 512):   # (the band rows are the same with FS_FLAG_SPECTRAL_IR: whatever flags the reconstruct had)
        env = install_envelopes(pkg, ctx, s, rng, flags)
        left, right = ctx.reverb_ear_impulse_responses(s)
        wl, wr = ear_irs(env, cm, cs)
        el, er = rel_rms(left, wl), rel_rms(right, wr)
        print(f"ear IRs ns={ns} B={B} flags={flags}: rel rms left {el:.3e} right {er:.3e}")
        assert el <= 1e-6 and er <= 1e-6, (el, er)
        if B > 1:
            assert rel_rms(left, wr) > 1e-2    # (the ears differ: a swap would show)
    # after fs_set_band_edges: the set is rebuilt for the new edges
    if B > 1:
        base = edges if edges is not None else [125.0 * 2.0 ** (b - 0.5) for b in range(1, B)]
        moved = [float(np.float32(e * 0.8)) for e in base]
        ctx.set_band_edges(moved)
        assert ctx.reverb_ears_info() == (radius, SPEED, True)
        cm2, cs2 = ear_carriers(B, ns, ns, radius, SPEED, moved)
        left, right = ctx.reverb_ear_impulse_responses(s)
        wl, wr = ear_irs(env, cm2, cs2)
        assert rel_rms(left, wl) <= 1e-6 and rel_rms(right, wr) <= 1e-6, (rel_rms(left, wl), rel_rms(right, wr))
        assert rel_rms(left, ear_irs(env, cm, cs)[0]) > 1e-3   # (the carriers did move)
        cm, cs = cm2, cs2
    # after fs_set_impulse_response: every band row is the installed IR
    ir = (rng.normal(0, 1, ns) * np.exp(-np.arange(ns) / (ns / 3.0)) * 0.004).astype(np.float32)
    ctx.set_impulse_response(s, ir)
    left, right = ctx.reverb_ear_impulse_responses(s)
    wl, wr = ear_irs(np.tile(ir, (B, 1)), cm, cs)
    assert rel_rms(left, wl) <= 1e-6 and rel_rms(right, wr) <= 1e-6, (rel_rms(left, wl), rel_rms(right, wr))
    ctx.close()


# ---- GPU 2: callback parity ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ns,frame,B", SHAPES)
def test_callback_parity(pkg, ns, frame, B):
    """independent noise in the two channels, K + 4 callbacks (the spectrum ring wraps), the literal tail on odd callbacks at
    (6000, 48); then the right channel silent: nothing of the left leaks into it beyond the tolerance"""
    K = -(-ns // frame)
    ctx, (s,), _, _ = make_ctx(pkg, ns, B)
    rng = np.random.default_rng(7 * ns + frame + B)
    install_envelopes(pkg, ctx, s, rng)
    left, right = ctx.reverb_ear_impulse_responses(s)
    ear_source(ctx, s, frame)
    x = noise_blocks(rng, K + 4, frame)
    _, want = check_stream(ctx, s, x, left, right, frame, literal_odd=(ns, frame) == (6000, 48), what=f"ns={ns} F={frame} B={B}")
    assert np.abs(want).max() > 0.02
    ctx.reverb_release(s)
    calls = min(K + 2, 24)
    x = noise_blocks(rng, calls, frame)
    x[:, 1::2] = 0.0
    y, want = check_stream(ctx, s, x, left, right, frame, what=f"ns={ns} F={frame} B={B} right silent")
    assert not want[:, 1::2].any() and np.abs(want[:, 0::2]).max() > 0.02
    ctx.close()


# ---- GPU 3: the coherent limit ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ns,frame,B", [(6000, 48, 3), (6000, 16, 8)])
def test_coherent_limit(pkg, ns, frame, B):
    ctx, (s,), _, _ = make_ctx(pkg, ns, B, radius=0.0)
    rng = np.random.default_rng(ns + B)
    install_envelopes(pkg, ctx, s, rng)
    left, right = ctx.reverb_ear_impulse_responses(s)
    assert left.any() and np.array_equal(left, right)
    ear_source(ctx, s, frame)
    x = noise_blocks(rng, 12, frame)
    x[:, 1::2] = x[:, 0::2]
    y, _ = check_stream(ctx, s, x, left, left, frame, what=f"coherent ns={ns} F={frame} B={B}")
    ctx.close()


# ---- GPU 4: crossfade ---------------------------------------------------------------------------------------------------------

NS_X, F_X, B_X = 6000, 64, 3


class EarsModel:
    """CrossfadeModel per ear: the left output of the model fed h_L, the right output of the one fed h_R"""

    def __init__(self, n, frame, fade_len):
        self.l, self.r = CrossfadeModel(n, frame, fade_len), CrossfadeModel(n, frame, fade_len)

    def install(self, left, right):
        self.l.install(left); self.r.install(right)

    def process(self, blk, literal=False):
        a, b = self.l.process(blk, literal=literal), self.r.process(blk, literal=literal)
        out = a.copy()
        out[1::2] = b[1::2]
        return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_frame", "across_callbacks", "fold"])
def test_crossfade_rules_per_ear(pkg, name):
    """test_reverb_partitioned.py::test_crossfade_rules' schedules: a one-frame fade; a fade across callbacks with the literal
    tail during it and several installs between two callbacks; an install cutting a fade short"""
    L, schedule = CROSSFADE_SCHEDULES[name]
    ctx, (s,), _, _ = make_ctx(pkg, NS_X, B_X)
    ear_source(ctx, s, F_X, fade=L)
    model = EarsModel(NS_X, F_X, L)
    rng = np.random.default_rng(len(name))
    for step, actions in enumerate(schedule):
        literal = False
        for act in actions:
            if act == "ir":
                install_envelopes(pkg, ctx, s, rng)
                model.install(*ctx.reverb_ear_impulse_responses(s))
            else:
                assert act == "literal"
                literal = True
        blk = noise_blocks(rng, 1, F_X)[0]
        got, want = ctx.reverb_process(s, blk, literal_tail=literal), model.process(blk, literal=literal)
        assert close(got, want), (step, actions, np.abs(got - want).max())
    ctx.close()


@pytest.mark.gpu
def test_replacing_the_set_goes_through_the_crossfade(pkg):
    """a new ear set bumps the generation: the source takes again at its next callback, fading from the pair it heard"""
    L = 200
    ctx, (s,), _, radius = make_ctx(pkg, NS_X, B_X)
    rng = np.random.default_rng(5)
    install_envelopes(pkg, ctx, s, rng)
    ear_source(ctx, s, F_X, fade=L)
    model = EarsModel(NS_X, F_X, L)
    model.install(*ctx.reverb_ear_impulse_responses(s))
    for c, blk in enumerate(noise_blocks(rng, 10, F_X)):
        if c == 3:
            ctx.reverb_ears_set(radius_cm=radius * 0.5)
            pair = ctx.reverb_ear_impulse_responses(s)
            assert not np.array_equal(pair[0], np.asarray(model.l.ir, np.float32))
            model.install(*pair)
        got, want = ctx.reverb_process(s, blk), model.process(blk)
        assert close(got, want), (c, np.abs(got - want).max())
    ctx.close()


# ---- GPU 5: to the bit --------------------------------------------------------------------------------------------------------

CALLS_B = 10


def drive(pkg, kinds, serve, ears_installed=True):
    """kinds[i]: 'ear', 'part' or 'direct'; serve(ctx, srcs, blocks, apply) per callback.  The sources are driven alike whatever
    serves them: source 0 fades, source 2 is bypassed in some callbacks, IRs change on the way."""
    ctx, srcs, _, _ = make_ctx(pkg, NS_X, B_X, count=len(kinds), ears=ears_installed)
    rng = np.random.default_rng(66)
    for s in srcs:
        install_envelopes(pkg, ctx, s, rng)
    for i, (s, k) in enumerate(zip(srcs, kinds)):
        if k != "direct":
            ctx.reverb_set_engine(s, PARTITIONED)
        ctx.reverb_set_ears(s, k == "ear")
        if i == 0:
            ctx.reverb_set_crossfade(s, 200)
        ctx.reverb_init(s, F_X)
    res = []
    for c in range(CALLS_B):
        if c in (2, 3, 7):
            install_envelopes(pkg, ctx, srcs[0], rng)
        if c == 5:
            install_envelopes(pkg, ctx, srcs[-1], rng)
        apply = [True] * len(kinds)
        apply[2] = c not in (4, 5, 8)
        res.append(serve(ctx, srcs, noise_blocks(rng, len(kinds), F_X), apply))
    ctx.close()
    return res


def serve_single(ctx, srcs, blk, apply):
    return np.stack([ctx.reverb_process(s, blk[i], apply_reverb=apply[i]) for i, s in enumerate(srcs)])


def serve_batch(ctx, srcs, blk, apply):
    return ctx.reverb_process_batch(srcs, blk, apply=apply, want_out=True, want_mix=True)


@pytest.mark.gpu
def test_one_call_or_several_to_the_bit(pkg):
    kinds = ("ear",) * 4
    single = drive(pkg, kinds, serve_single)
    both = drive(pkg, kinds, serve_batch)
    assert max(np.abs(o).max() for o in single) > 0.02
    for c in range(CALLS_B):
        out, mix = both[c]
        assert np.array_equal(out, single[c]), c
        want = out[0].copy()
        for r in range(1, 4):
            want = want + out[r]   # fp32, list order
        assert np.array_equal(mix, want), c
        assert not np.array_equal(out[0][0::2], out[0][1::2])


@pytest.mark.gpu
def test_other_rows_keep_their_bits(pkg):
    """[ear, partitioned, direct, ear, partitioned, direct] in one batch: every row without ears — and, through the later
    callbacks, its state — is that of the same schedule in a context where no ear set was ever installed (there the two ear
    sources are plain partitioned ones)"""
    kinds = ("ear", "part", "direct", "ear", "part", "direct")
    plain = tuple("part" if k == "ear" else k for k in kinds)
    with_ears = drive(pkg, kinds, serve_batch)
    without = drive(pkg, plain, serve_batch, ears_installed=False)
    for c in range(CALLS_B):
        for r, k in enumerate(kinds):
            if k == "ear":
                assert not np.array_equal(with_ears[c][0][r], without[c][0][r]), (c, r)
            else:
                assert np.array_equal(with_ears[c][0][r], without[c][0][r]), (c, r)


# ---- GPU 6: traced IRs and the threads ------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_traced_irs_and_the_threads(pkg, scene_factory):
    """starter_room, 4 bands, 4096 rays: an ear callback after each tick against the ear IRs of that tick; then an audio thread
    of ear callbacks beside a game thread that reconstructs two frames' energies in turn — every reconstruct is a newer IR, so
    callbacks keep taking: every block must be the convolution with one of the two pairs, whichever was current"""
    frame = 1024
    sc = scene_factory("starter_room", 4)
    ctx = pkg.Context(num_bands=4)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    ctx.reverb_ears_set()
    s = ctx.create_source(sc.source)
    ear_source(ctx, s, frame)
    model = EarsModel(ctx.num_samples, frame, 0)
    rng = np.random.default_rng(9)
    for tick in range(3):
        ctx.update_sources([s], traced_params(pkg, 300 + tick, rays=4096))
        pair = ctx.reverb_ear_impulse_responses(s)
        assert pair[0].any() and not np.array_equal(pair[0], pair[1])
        model.install(*pair)
        for blk in noise_blocks(rng, 2, frame):   # the second callback takes nothing: its own spectra
            got, want = ctx.reverb_process(s, blk), model.process(blk)
            assert close(got, want), (tick, np.abs(got - want).max())

    # two different frames' energies, reconstructed in turn by the game thread: the band rows a take reads really change under
    # it, so a take that read them while a reconstruct wrote them would give a block that matches neither pair
    energies, pairs = [], []
    for tick in (0, 1):
        ctx.update_sources([s], traced_params(pkg, 400 + tick, rays=4096))
        energies.append(ctx.energy_buffer(s).copy())
    for e in energies:
        ctx.update_energy_buffer(s, e)
        ctx.reconstruct_impulse_response(s, pkg.default_params())
        pairs.append(ctx.reverb_ear_impulse_responses(s))
    assert pairs[0][0].any() and not np.array_equal(pairs[0][0], pairs[1][0])
    models = [copy.deepcopy(model), copy.deepcopy(model)]   # (the history so far; with no fade length a model convolves what is installed)
    for m, pair in zip(models, pairs):
        m.install(*pair)
    done = threading.Event()
    errors, ins, outs = [], [], []

    def audio():
        arng = np.random.default_rng(60)
        try:
            while (not done.is_set() or len(outs) < 20) and len(outs) < 60:
                blk = noise_blocks(arng, 1, frame)[0]
                outs.append(ctx.reverb_process(s, blk))
                ins.append(blk)
        except Exception as e:     # noqa: BLE001 — reported below
            errors.append(e)

    t = threading.Thread(target=audio)
    t.start()
    try:
        for k in range(40):
            ctx.update_energy_buffer(s, energies[k % 2])
            ctx.reconstruct_impulse_response(s, pkg.default_params())
    finally:
        done.set()
        t.join()
    assert not errors, errors
    assert len(outs) >= 20
    after = ctx.reverb_ear_impulse_responses(s)
    assert np.array_equal(after[0], pairs[1][0]) and np.array_equal(after[1], pairs[1][1])
    seen = [0, 0]
    for c, (blk, got) in enumerate(zip(ins, outs)):
        wants = [m.process(blk) for m in models]
        ok = [bool(close(got, w)) for w in wants]
        assert ok[0] or ok[1], (c, [np.abs(got - w).max() for w in wants])
        seen[0] += ok[0]; seen[1] += ok[1]
    print(f"ears threads: {len(outs)} callbacks, {seen[0]} with the first pair and {seen[1]} with the second")
    ctx.close()


# ---- GPU 7: refusals change nothing -------------------------------------------------------------------------------------------

def refused(pkg, ctx, call, *needles):
    with pytest.raises(pkg.FrequenSeeError) as ei:
        call()
    assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT, ei.value
    for n in needles:
        assert n in str(ei.value), (n, str(ei.value))


def refusal_run(pkg, disturb):
    """an ear source's callbacks with `disturb(ctx, s, other)` between them (None: the undisturbed run)"""
    ctx, (s, other), _, radius = make_ctx(pkg, NS_X, B_X, count=2)
    rng = np.random.default_rng(21)
    install_envelopes(pkg, ctx, s, rng)
    ear_source(ctx, s, F_X)
    x = noise_blocks(rng, 6, F_X)
    out = []
    for c in range(6):
        if c in (2, 4) and disturb is not None:
            disturb(ctx, s, other)
            assert ctx.reverb_ears_info() == (radius, SPEED, True)
        out.append(ctx.reverb_process(s, x[c]))
    ctx.close()
    return np.stack(out)


_undisturbed = {}


def undisturbed(pkg):
    if "out" not in _undisturbed:
        out = refusal_run(pkg, None)
        out.setflags(write=False)
        _undisturbed["out"] = out
    return _undisturbed["out"]


def set_desc(pkg, ctx, **kw):
    d = pkg._capi.default_reverb_ears(**kw)
    ctx.check(ctx.lib.fs_reverb_ears_set(ctx.h, C.byref(d)))


REFUSALS = {
    "ears_under_the_direct_engine":
        lambda pkg, ctx, s, o: (ctx.reverb_set_engine(o, DIRECT), ctx.reverb_set_ears(o, True),
                                refused(pkg, ctx, lambda: ctx.reverb_init(o, F_X), "FS_REVERB_ENGINE_PARTITIONED")),
    "clearing_under_an_ear_source":
        lambda pkg, ctx, s, o: refused(pkg, ctx, lambda: ctx.reverb_ears_set(clear=True), "cleared", "initialised with ears"),
    "wrong_struct_size":
        lambda pkg, ctx, s, o: refused(pkg, ctx, lambda: set_desc(pkg, ctx, struct_size=8), "struct_size"),
    "nan_radius":
        lambda pkg, ctx, s, o: refused(pkg, ctx, lambda: set_desc(pkg, ctx, radius_cm=float("nan")), "radius_cm"),
    "negative_radius":
        lambda pkg, ctx, s, o: refused(pkg, ctx, lambda: set_desc(pkg, ctx, radius_cm=-1.0), "radius_cm"),
    "nan_sound_speed":
        lambda pkg, ctx, s, o: refused(pkg, ctx, lambda: set_desc(pkg, ctx, sound_speed_cm_s=float("nan")), "sound_speed_cm_s"),
    "a_band_without_a_bin":
        lambda pkg, ctx, s, o: refused(pkg, ctx, lambda: ctx.set_band_edges([100.0, 100.1]), "fs_set_band_edges", "at least one FFT bin"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_change_nothing(pkg, name):
    got = refusal_run(pkg, lambda ctx, s, o: REFUSALS[name](pkg, ctx, s, o))
    assert np.array_equal(got, undisturbed(pkg)), name


@pytest.mark.gpu
def test_refusals_without_a_set(pkg):
    """ears on with no set installed; a set whose band edges leave a band without a bin (the default octave edges at 6 kHz);
    the copy without a set — then the good calls, and the callback of the undisturbed run"""
    ctx = pkg.Context(num_bands=B_X, sample_rate=NS_X, simulated_duration=1.0)
    s, _ = [ctx.create_source((0.0, 0.0, 0.0)) for _ in range(2)]
    assert ctx.reverb_ears_info() == (0.0, 0.0, False)
    ctx.reverb_ears_set(clear=True)                      # nothing to clear: fine
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_set_ears(s, True)
    refused(pkg, ctx, lambda: ctx.reverb_init(s, F_X), "no ear set is installed")
    refused(pkg, ctx, lambda: ctx.reverb_ear_impulse_responses(s), "no ear set is installed")
    ctx2 = pkg.Context(num_bands=8, sample_rate=NS_X, simulated_duration=1.0)
    refused(pkg, ctx2, lambda: ctx2.reverb_ears_set(), "fs_reverb_ears_set", "at least one FFT bin")
    assert ctx2.reverb_ears_info() == (0.0, 0.0, False)
    ctx2.close()
    ctx.set_band_edges(edges_for(B_X, NS_X))
    ctx.reverb_ears_set(radius_cm=radius_for(NS_X))
    rng = np.random.default_rng(21)
    install_envelopes(pkg, ctx, s, rng)
    ctx.reverb_init(s, F_X)                              # (the recorded choices held through the refusals)
    x = noise_blocks(rng, 6, F_X)
    got = np.stack([ctx.reverb_process(s, x[c]) for c in range(6)])
    assert np.array_equal(got, undisturbed(pkg))
    ctx.reverb_set_ears(s, False)                        # without ears again: the set can go
    ctx.reverb_init(s, F_X)
    ctx.reverb_ears_set(clear=True)
    assert ctx.reverb_ears_info() == (0.0, 0.0, False)
    ctx.close()


@pytest.mark.gpu
def test_plugin_switch(pkg):
    sub = pkg.AudioRayTracingSubsystem(num_bands=1, device=0)
    comp = pkg.FrequenSeeAudioComponent((0.0, 0.0, 0.0))
    comp.OnRegister(sub)
    sub.ctx.reverb_ears_set()
    plug = pkg.FrequenSeeAudioReverbPlugin(sub)
    plug.Initialize(256)
    plug.Ears = True
    plug.OnInitSource(comp)
    ir = np.zeros(sub.ctx.num_samples, np.float32)
    ir[0] = 0.5
    sub.ctx.set_impulse_response(comp._src, ir)
    left, right = sub.ctx.reverb_ear_impulse_responses(comp._src)
    x = noise_blocks(np.random.default_rng(3), 1, 256)[0]
    y = plug.ProcessSourceAudio(comp, x)
    want = np.empty_like(x, dtype=np.float64)
    want[0::2], want[1::2] = float(left[0]) * x[0::2], float(right[0]) * x[1::2]
    assert close(y, want) and left[0] != right[0]
    sub.Deinitialize()


@pytest.mark.gpu
def test_cpp_mirror_plugin(pkg, tmp_path):
    """host/FrequenSee.hpp's FrequenSeeAudioReverbPlugin through the headless harness: SetEars, OnInitSource, one callback of a
    half-scale unit impulse and EarImpulseResponses — the block is 0.5 h_L | 0.5 h_R within the engine's tolerance"""
    import json
    import subprocess
    exe = os.path.join(os.path.dirname(pkg._capi.LIB_PATH), "fs_harness")
    r = subprocess.run([exe, "1", "256", "2", str(tmp_path / "ir.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert j["ears_peak"] > 0.01 and j["ears_left_right_max_diff"] > 1e-3, j
    assert j["ears_max_err"] <= TOL * max(j["ears_peak"], 1e-3), j
