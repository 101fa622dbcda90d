"""fs_reverb_set_crossfade: the reverb callback fades between successive impulse responses instead of switching at a block
boundary (include/frequensee.h, rules 1-5 beside fs_reverb_process).  The expected outputs come from a float64 restatement
of those rules (CrossfadeModel) over the tracked per-channel history, convolved through the FFT as in
test_reverb.py::test_fft_product_equals_direct_convolution."""
import threading

import numpy as np
import pytest

FRAME = 1024
TOL = 2e-5          # test_reverb.py: |got - want| <= 2e-5 * max(|want|, 1e-3)
SPECTRAL = 512      # FS_FLAG_SPECTRAL_IR


def conv_block(h, u, n, frame):
    """y[s] = sum_k h[k] u[n - 1 + s - k], s < frame (u = the n - 1 history samples, then the block)"""
    m = 1 << int(np.ceil(np.log2(n + u.shape[0])))
    return np.fft.irfft(np.fft.rfft(h, m) * np.fft.rfft(u, m), m)[n - 1:n - 1 + frame]


class CrossfadeModel:
    """One source's reverb callback with fs_reverb_set_crossfade, in float64."""

    def __init__(self, n, frame, fade_len=0):
        self.n, self.frame, self.L = n, frame, fade_len
        self.hist = np.zeros((2, n - 1))
        self.ir = np.zeros(n)          # the device IR (zero until the first install)
        self.new = False               # the device IR is newer than h_to (rule 1: only the newest counts)
        self.h_from = self.h_to = None
        self.fading, self.pos, self.primed = False, 0, False

    def install(self, ir):
        self.ir = np.asarray(ir, np.float64).copy()
        self.new = True

    def set_crossfade(self, fade_len):
        if self.L == 0:
            self.primed = False        # rule 4: enabling takes the IR unfaded
        self.fading = False            # a running fade ends at its target
        self.L = fade_len

    def release(self):
        self.hist[:] = 0.0
        self.fading = False

    def gains(self):
        p = self.pos + np.arange(self.frame)
        return np.where(p < self.L, (p + 1) / max(self.L, 1), 1.0)

    def process(self, block, literal=False):
        f, n = self.frame, self.n
        b = np.asarray(block, np.float64)
        x = [b[:f], b[:f]] if literal else [b[0::2], b[1::2]]
        u = [np.concatenate([self.hist[c], x[c]]) for c in range(2)]
        self.hist = np.stack([np.concatenate([self.hist[c], b[c::2]])[f:] for c in range(2)])
        if self.L == 0:
            y = [conv_block(self.ir, u[c], n, f) for c in range(2)]
        else:
            if not self.primed:
                self.h_to, self.fading, self.primed = self.ir.copy(), False, True
            elif self.new:
                if self.fading:                                   # rule 3
                    a = self.pos / self.L
                    self.h_from = (1 - a) * self.h_from + a * self.h_to
                else:
                    self.h_from = self.h_to
                self.h_to, self.fading, self.pos = self.ir.copy(), True, 0
            self.new = False
            if self.fading:                                       # rule 2
                g = self.gains()
                y = [(1 - g) * conv_block(self.h_from, u[c], n, f) + g * conv_block(self.h_to, u[c], n, f) for c in range(2)]
                self.pos += f
                if self.pos >= self.L:
                    self.fading = False
            else:
                y = [conv_block(self.h_to, u[c], n, f) for c in range(2)]
        out = np.empty(2 * f)
        out[0::2], out[1::2] = y[0], y[1]
        return np.clip(out, -1.0, 1.0)


def blocks(rng, n, frame=FRAME):
    return [np.clip(rng.normal(0, 0.3, 2 * frame), -1, 1).astype(np.float32) for _ in range(n)]


def noise_ir(rng, n, decay=5000.0, gain=0.02):
    return (rng.normal(0, 1, n) * np.exp(-np.arange(n) / decay) * gain).astype(np.float32)


def close(got, want):
    return np.abs(got - want).max() <= TOL * max(np.abs(want).max(), 1e-3)


# ---- CPU: the entry point and the restatement's own invariants ------------------------------------------------------------

def test_entry_point_exported_and_bound(pkg):
    assert "fs_reverb_set_crossfade" in pkg._capi.EXPORTS
    lib = pkg._capi.load()
    assert hasattr(lib, "fs_reverb_set_crossfade")
    assert lib.fs_reverb_set_crossfade.argtypes is not None and len(lib.fs_reverb_set_crossfade.argtypes) == 3
    assert hasattr(pkg.Context, "reverb_set_crossfade") and hasattr(pkg.FrequenSeeAudioReverbPlugin, "SetCrossfade")


def test_null_context_is_an_invalid_argument(pkg):
    lib = pkg._capi.load()
    assert lib.fs_reverb_set_crossfade(None, 0, 256) == pkg._capi.ERR_INVALID_ARGUMENT
    assert lib.fs_reverb_set_crossfade(None, 0, 0) == pkg._capi.ERR_INVALID_ARGUMENT


N_CPU, F_CPU = 3000, 256


def test_model_fade_of_one_sample_is_the_abrupt_switch():
    """L = 1: g_0 = 1, the new IR from the block's first sample — the default path's switch"""
    rng = np.random.default_rng(1)
    fade, plain = CrossfadeModel(N_CPU, F_CPU, 1), CrossfadeModel(N_CPU, F_CPU, 0)
    for i, b in enumerate(blocks(rng, 8, F_CPU)):
        if i in (0, 2, 3, 6):
            ir = noise_ir(rng, N_CPU, 600.0, 0.05)
            fade.install(ir); plain.install(ir)
        assert np.allclose(fade.process(b), plain.process(b), rtol=0, atol=1e-12), i


def test_model_equal_irs_make_the_fade_a_no_op():
    rng = np.random.default_rng(2)
    ir = noise_ir(rng, N_CPU, 600.0, 0.05)
    fade, plain = CrossfadeModel(N_CPU, F_CPU, 700), CrossfadeModel(N_CPU, F_CPU, 0)
    fade.install(ir); plain.install(ir)
    for i, b in enumerate(blocks(rng, 8, F_CPU)):
        if i in (1, 2, 5):
            fade.install(ir)          # a new generation of the same IR: a fade that changes nothing
        assert np.allclose(fade.process(b), plain.process(b), rtol=0, atol=1e-12), i
    assert fade.primed and not fade.fading


def test_model_mid_fade_mix_equals_separate_convolutions():
    """rule 3 is exact: convolving the mixed IR equals mixing the two IRs' outputs"""
    rng = np.random.default_rng(3)
    h1, h2 = noise_ir(rng, N_CPU, 600.0).astype(np.float64), noise_ir(rng, N_CPU, 600.0).astype(np.float64)
    u = rng.normal(0, 0.3, N_CPU - 1 + F_CPU)
    for a in (0.0, 0.25, 700 / 1100, 1.0):
        mixed = conv_block((1 - a) * h1 + a * h2, u, N_CPU, F_CPU)
        separate = (1 - a) * conv_block(h1, u, N_CPU, F_CPU) + a * conv_block(h2, u, N_CPU, F_CPU)
        assert np.abs(mixed - separate).max() < 1e-12
    # and the direct sum agrees with the FFT form
    s = np.array([np.dot(h1, u[t:t + N_CPU][::-1]) for t in range(F_CPU)])
    assert np.abs(conv_block(h1, u, N_CPU, F_CPU) - s).max() < 1e-12
    # a fade cut short at p0 continues from the IR heard at its last output sample
    m = CrossfadeModel(N_CPU, F_CPU, 700)
    m.install(h1); m.process(np.zeros(2 * F_CPU))
    m.install(h2); m.process(np.zeros(2 * F_CPU)); m.process(np.zeros(2 * F_CPU))
    assert m.fading and m.pos == 2 * F_CPU
    h3 = noise_ir(rng, N_CPU, 600.0).astype(np.float64)
    m.install(h3); m.process(np.zeros(2 * F_CPU))
    a = 2 * F_CPU / 700
    assert np.abs(m.h_from - ((1 - a) * h1 + a * h2)).max() < 1e-15 and np.array_equal(m.h_to, h3)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def installed_ctx(pkg, count=1):
    ctx = pkg.Context(num_bands=1)
    return ctx, [ctx.create_source(np.zeros(3, np.float32)) for _ in range(count)]


@pytest.mark.gpu
def test_argument_checks(pkg):
    ctx, (s,) = installed_ctx(pkg)
    sr = ctx.cfg.sample_rate
    for bad in (-1, 4 * sr + 1, -(1 << 31)):
        with pytest.raises(pkg.FrequenSeeError) as e:
            ctx.reverb_set_crossfade(s, bad)
        assert e.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    with pytest.raises(pkg.FrequenSeeError) as e:
        ctx.reverb_set_crossfade(s + 17, 256)
    assert e.value.code == pkg._capi.ERR_BAD_HANDLE
    for ok in (0, 1, 4 * sr, 0):
        ctx.reverb_set_crossfade(s, ok)
    ctx.close()


@pytest.mark.gpu
def test_set_then_reset_is_bit_identical_to_never_set(pkg):
    ctx, (a, b, c) = installed_ctx(pkg, 3)
    ctx.reverb_set_crossfade(c, 2560)                   # set and reset before the first callback
    ctx.reverb_set_crossfade(c, 0)
    for s in (a, b, c):
        ctx.reverb_init(s, FRAME)
    ctx.reverb_set_crossfade(b, 2560)                   # set after fs_reverb_init, used, then reset mid-fade
    model = CrossfadeModel(ctx.num_samples, FRAME, 0)
    rng = np.random.default_rng(10)
    changes = {0, 1, 4, 5, 7, 9}
    for i, blk in enumerate(blocks(rng, 12)):
        if i in changes:
            ir = noise_ir(rng, ctx.num_samples)
            for s in (a, b, c):
                ctx.set_impulse_response(s, ir)
            model.install(ir)
        if i == 6:
            ctx.reverb_set_crossfade(b, 0)
        ya, yb, yc = (ctx.reverb_process(s, blk) for s in (a, b, c))
        assert np.array_equal(ya, yc), i
        assert close(ya, model.process(blk)), i
        if i >= 6:
            assert np.array_equal(ya, yb), i
        elif i == 5:
            assert not np.array_equal(ya, yb), "the crossfade changed nothing mid-fade"
    ctx.close()


def run_schedule(pkg, ctx, s, model, schedule, rng):
    """schedule: per callback a list of actions before it ('ir', 'release', ('literal',), ('L', n))"""
    outs = []
    for step, actions in enumerate(schedule):
        literal = False
        for act in actions:
            if act == "ir":
                ir = noise_ir(rng, ctx.num_samples, decay=float(rng.uniform(2000, 8000)))
                ctx.set_impulse_response(s, ir)
                model.install(ir)
            elif act == "release":
                ctx.reverb_release(s)
                model.release()
            elif act == "literal":
                literal = True
            elif isinstance(act, tuple) and act[0] == "L":
                ctx.reverb_set_crossfade(s, act[1])
                model.set_crossfade(act[1])
        blk = blocks(rng, 1)[0]
        got = ctx.reverb_process(s, blk, literal_tail=literal)
        want = model.process(blk, literal=literal)
        assert close(got, want), (step, np.abs(got - want).max())
        outs.append(got)
    return outs


@pytest.mark.gpu
def test_fade_over_one_frame(pkg):
    """L = frame: the blocks before, during and after one change"""
    ctx, (s, ref) = installed_ctx(pkg, 2)
    ctx.reverb_set_crossfade(s, FRAME)                  # (set before fs_reverb_init)
    ctx.reverb_init(s, FRAME)
    ctx.reverb_init(ref, FRAME)
    rng = np.random.default_rng(20)
    model = CrossfadeModel(ctx.num_samples, FRAME, FRAME)
    ir1, ir2 = noise_ir(rng, ctx.num_samples), noise_ir(rng, ctx.num_samples)
    ctx.set_impulse_response(s, ir1); ctx.set_impulse_response(ref, ir1); model.install(ir1)
    for step in range(5):
        if step == 2:
            ctx.set_impulse_response(s, ir2); ctx.set_impulse_response(ref, ir2); model.install(ir2)
        blk = blocks(rng, 1)[0]
        got, abrupt = ctx.reverb_process(s, blk), ctx.reverb_process(ref, blk)
        want = model.process(blk)
        assert close(got, want), step
        if step == 2:
            assert model.fading is False and model.pos == FRAME    # the fade lasted exactly this block
            assert not np.allclose(got, abrupt, atol=1e-4)          # ... and it is not the abrupt switch
        else:
            assert close(got, abrupt), step                         # no fade running: the plain convolution
    ctx.close()


@pytest.mark.gpu
def test_fade_across_callbacks(pkg):
    """L = 2560, not a multiple of the frame: a third IR mid-fade, three installs between two callbacks, the literal
    tail during a fade, a release mid-fade, a new fade length mid-fade"""
    ctx, (s,) = installed_ctx(pkg)
    ctx.reverb_init(s, FRAME)
    ctx.reverb_set_crossfade(s, 2560)
    model = CrossfadeModel(ctx.num_samples, FRAME, 2560)
    rng = np.random.default_rng(30)
    schedule = [
        ["ir"], [], ["ir"], [],                          # a fade starts; 1024 samples in
        ["ir"], [], [], [], [],                          # rule 3: a third IR at p0 = 2048; the new fade runs out
        ["ir", "ir", "ir"], [], [],                      # three installs between two callbacks: only the newest counts
        ["ir"], ["literal"], ["literal"], [],            # the literal tail during a fade
        ["ir"], ["release"], [], ["ir"], [],             # release mid-fade: ends the fade at its target
        ["ir"], [("L", 700)], ["ir"], [], [],            # a new length ends the running fade; the next one is 700 long
        [("L", 0)], ["ir"], [("L", 2560)], ["ir"], [],   # off, then on again: the first callback takes the IR unfaded
    ]
    run_schedule(pkg, ctx, s, model, schedule, rng)
    ctx.close()


@pytest.mark.gpu
def test_bypass_touches_no_fade_state(pkg):
    ctx, (s,) = installed_ctx(pkg)
    ctx.reverb_init(s, FRAME)
    ctx.reverb_set_crossfade(s, 2560)
    model = CrossfadeModel(ctx.num_samples, FRAME, 2560)
    rng = np.random.default_rng(40)
    run_schedule(pkg, ctx, s, model, [["ir"], ["ir"]], rng)           # a fade 1024 samples in
    ir = noise_ir(rng, ctx.num_samples)
    ctx.set_impulse_response(s, ir)
    model.install(ir)
    blk = blocks(rng, 1)[0]
    assert np.array_equal(ctx.reverb_process(s, blk, apply_reverb=False), blk)
    run_schedule(pkg, ctx, s, model, [[], [], []], rng)              # the fade continues where it was (no history pushed)
    ctx.close()


def traced_ctx(pkg, sc):
    ctx = pkg.Context(num_bands=4)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    s = ctx.create_source(sc.source)
    ctx.reverb_init(s, FRAME)
    ctx.reverb_set_crossfade(s, 2560)
    return ctx, s


def traced_params(pkg, seed, flags=0, rays=8192):
    return pkg.default_params(num_rays=rays, depth=8, seed=seed, dist_divisor=100.0, flags=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["update_sources", "update_sources_spectral", "batch_async", "pipelined"])
def test_traced_irs_every_route(pkg, scene_factory, route):
    """1000-pair-class traced IRs on starter_room, through every route that rewrites the device IR; the expected IR is the
    published one (fs_copy_impulse_response) after each producer call"""
    sc = scene_factory("starter_room", 4)
    ctx, s = traced_ctx(pkg, sc)
    if route == "pipelined":
        ctx.set_pipelining(2)
        ctx.set_frames_per_launch(2)
    model = CrossfadeModel(ctx.num_samples, FRAME, 2560)
    rng = np.random.default_rng(50)
    prev = None
    seed = 100
    for step in range(7):
        produce = step != 3                             # one callback without a new IR (the fade goes on)
        if produce:
            if route.startswith("update_sources"):
                ctx.update_sources([s], traced_params(pkg, seed, SPECTRAL if route.endswith("spectral") else 0))
                seed += 1
            elif route == "batch_async":
                p = traced_params(pkg, seed); seed += 1
                ctx.compute_energy_response_batch_async([s], p)
                ctx.reconstruct_impulse_response_batch_async([s], p)
                ctx.synchronize()
            else:                                       # two frames of the stream per callback: only the newer counts
                for _ in range(2):
                    p = traced_params(pkg, seed); seed += 1
                    ctx.compute_energy_response_async(s, p)
                    ctx.reconstruct_impulse_response_async(s, p)
                ctx.synchronize()
            ir = ctx.impulse_response(s, 0)
            assert ir.any()
            if prev is not None:
                assert not np.array_equal(ir, prev)    # a different IR every tick: a fade every time
            prev = ir
            model.install(ir)
        blk = blocks(rng, 1)[0]
        got = ctx.reverb_process(s, blk)
        want = model.process(blk)
        assert close(got, want), (route, step, np.abs(got - want).max())
    ctx.close()


@pytest.mark.gpu
def test_audio_thread_against_game_thread(pkg, scene_factory):
    """crossfaded callbacks on one thread while another runs 200 ticks of fs_update_sources"""
    sc = scene_factory("starter_room", 4)
    ctx, s = traced_ctx(pkg, sc)
    done = threading.Event()
    errors, peak, count = [], [0.0], [0]

    def audio():
        rng = np.random.default_rng(60)
        try:
            while not done.is_set() or count[0] < 20:
                y = ctx.reverb_process(s, blocks(rng, 1)[0])
                if not np.isfinite(y).all():
                    raise AssertionError(f"callback {count[0]}: a non-finite sample")
                peak[0] = max(peak[0], float(np.abs(y).max()))
                count[0] += 1
        except Exception as e:     # noqa: BLE001 — reported below
            errors.append(e)

    t = threading.Thread(target=audio)
    t.start()
    try:
        for tick in range(200):
            ctx.update_sources([s], traced_params(pkg, 1000 + tick, rays=4096))
    finally:
        done.set()
        t.join()
    assert not errors, errors
    assert count[0] >= 20 and 0.0 < peak[0] <= 1.0
    ctx.close()
