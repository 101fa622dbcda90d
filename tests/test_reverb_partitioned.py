"""fs_reverb_set_engine: the reverb callback's partitioned-FFT engine beside the direct one (include/frequensee.h, beside
fs_reverb_set_crossfade).  Expected values are float64 convolutions of the tracked per-channel stream — for fades the float64
model of test_reverb_crossfade.py — and the tolerance is the direct engine's: |got - want| <= 2e-5 * max(max|want|, 1e-3).
The engine's own arithmetic (complex64 transforms, fp32 accumulation over the partitions) is off the float64 convolution by
1 - 2e-7 of max(1, max|want|) at these shapes, two orders of magnitude inside that.

Contexts are sized like test_config_shapes.py::test_reverb_convolution: sample_rate = ns, one second, one band."""
import os
import re
import threading

import numpy as np
import pytest

from test_reverb_crossfade import TOL, CrossfadeModel, close, noise_ir, traced_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, PARTITIONED = 0, 1


# ---- CPU: the entry point ---------------------------------------------------------------------------------------------------

def test_entry_point_exported_bound_and_listed(pkg):
    assert "fs_reverb_set_engine" in pkg._capi.EXPORTS
    lib = pkg._capi.load()
    assert hasattr(lib, "fs_reverb_set_engine")
    assert lib.fs_reverb_set_engine.argtypes is not None and len(lib.fs_reverb_set_engine.argtypes) == 3
    assert hasattr(pkg.Context, "reverb_set_engine") and hasattr(pkg.FrequenSeeAudioReverbPlugin, "SetEngine")
    assert (pkg._capi.REVERB_ENGINE_DIRECT, pkg._capi.REVERB_ENGINE_PARTITIONED) == (DIRECT, PARTITIONED)
    header = open(os.path.join(ROOT, "include", "frequensee.h")).read()
    head = header[:header.index("#ifndef")]
    ext = set(re.findall(r"fs_[a-z0-9_]+", head[head.index("EXTENDED:"):head.index("(tests/test_capi_cpu.py")]))
    assert "fs_reverb_set_engine" in ext
    assert re.search(r"#define FS_REVERB_ENGINE_DIRECT\s+0\b", header) and re.search(r"#define FS_REVERB_ENGINE_PARTITIONED\s+1\b", header)


def test_null_context_is_an_invalid_argument(pkg):
    lib = pkg._capi.load()
    for engine in (DIRECT, PARTITIONED, 2):
        assert lib.fs_reverb_set_engine(None, 0, engine) == pkg._capi.ERR_INVALID_ARGUMENT


# ---- helpers ------------------------------------------------------------------------------------------------------------------

def make_ctx(pkg, ns, count=1):
    ctx = pkg.Context(num_bands=1, sample_rate=ns, simulated_duration=1.0)
    assert ctx.num_samples == ns
    return ctx, [ctx.create_source((0.0, 0.0, 0.0)) for _ in range(count)]


def shaped_ir(rng, ns):
    """test_reverb_convolution's IR: decaying noise, a strong first tap and a last tap that reads the far end of the history"""
    ir = (rng.normal(0, 1, ns) * np.exp(-np.arange(ns) / (ns / 3.0)) * 0.004).astype(np.float32)
    ir[0] = 0.25
    ir[-1] = 0.1
    return ir


def noise_blocks(rng, calls, frame):
    return np.clip(rng.normal(0, 0.3, (calls, 2 * frame)), -1, 1).astype(np.float32)


def conv_f64(x, h, n):
    m = 1
    while m < len(x) + len(h):
        m *= 2
    return np.fft.irfft(np.fft.rfft(x, m) * np.fft.rfft(h, m), m)[:n]


def expected_stream(x, ir, frame):
    """[calls][2 * frame] in float64: the convolution of each channel's whole stream, odd callbacks with the literal tail
    (RVB.cpp:147-148: the current block is the interleaved buffer's first `frame` floats; the history keeps the true samples)"""
    calls = x.shape[0]
    h = ir.astype(np.float64)
    want = np.empty((calls, 2 * frame))
    for ch in range(2):
        stream = x[:, ch::2].astype(np.float64).reshape(-1)
        w = conv_f64(stream, h, stream.size).reshape(calls, frame)
        for c in range(1, calls, 2):
            d = x[c, :frame].astype(np.float64) - x[c, ch::2].astype(np.float64)
            w[c] += conv_f64(d, h[:frame], frame)
        want[:, ch::2] = w
    return np.clip(want, -1.0, 1.0)


def parity_run(pkg, ns, frame, calls, seed):
    ctx, (s,) = make_ctx(pkg, ns)
    rng = np.random.default_rng(seed)
    ir = shaped_ir(rng, ns)
    ctx.set_impulse_response(s, ir)
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_init(s, frame)
    x = noise_blocks(rng, calls, frame)
    y = np.stack([ctx.reverb_process(s, x[c], literal_tail=bool(c % 2)) for c in range(calls)])
    want = expected_stream(x, ir, frame)
    worst = max(np.abs(y[c] - want[c]).max() / (TOL * max(np.abs(want[c]).max(), 1e-3)) for c in range(calls))
    print(f"partitioned parity ns={ns} frame={frame} calls={calls}: largest error = {worst:.4f} of the tolerance")
    for c in range(calls):
        assert close(y[c], want[c]), (c, np.abs(y[c] - want[c]).max())
    return ctx, s


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ns,frame", [(6000, 48), (6000, 16), (4097, 64), (1000, 1024), (12000, 2048), (48000, 1024)])
def test_parity_over_the_shapes(pkg, ns, frame):
    """N > 2F, the smallest frame, a last partition of one tap, an IR shorter than a frame, the largest frame, the default;
    until the spectrum ring has wrapped, the literal tail on odd callbacks; then release: silence in, silence out"""
    K = -(-ns // frame)
    ctx, s = parity_run(pkg, ns, frame, K + 4, 1000 * frame + ns)
    ctx.reverb_release(s)
    assert not ctx.reverb_process(s, np.zeros(2 * frame, np.float32)).any()
    ctx.close()


@pytest.mark.gpu
def test_beyond_the_ring(pkg):
    """an IR of 65 538 samples: refused by the direct engine (its history ring), convolved by the partitioned one"""
    ctx, (s,) = make_ctx(pkg, 65538)
    with pytest.raises(pkg.FrequenSeeError) as ei:
        ctx.reverb_init(s, 1024)
    assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    ctx.close()
    ctx, s = parity_run(pkg, 65538, 1024, 70, 65538)
    ctx.close()


@pytest.mark.gpu
def test_init_bounds_under_the_engine(pkg):
    ctx, (s,) = make_ctx(pkg, 6000)
    ctx.reverb_set_engine(s, PARTITIONED)
    for bad in (15, 2049, 0, -1):
        with pytest.raises(pkg.FrequenSeeError) as ei:
            ctx.reverb_init(s, bad)
        assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    for ok in (16, 2048):
        ctx.reverb_init(s, ok)
        assert ctx.reverb_process(s, np.zeros(2 * ok, np.float32)).shape == (2 * ok,)
    ctx.close()


@pytest.mark.gpu
def test_ir_replaced_between_callbacks(pkg):
    """no crossfade: the callback after a new IR convolves the whole history with it"""
    ns, frame = 6000, 64
    ctx, (s,) = make_ctx(pkg, ns)
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_init(s, frame)
    model = CrossfadeModel(ns, frame, 0)
    rng = np.random.default_rng(4)
    for c, blk in enumerate(noise_blocks(rng, 10, frame)):
        if c in (0, 3, 7):
            ir = noise_ir(rng, ns, 600.0, 0.05)
            ctx.set_impulse_response(s, ir)
            model.install(ir)
        got, want = ctx.reverb_process(s, blk), model.process(blk)
        assert close(got, want), (c, np.abs(got - want).max())
    ctx.close()


NS_X, F_X = 6000, 64


def run_schedule(ctx, s, model, schedule, rng, frame=F_X):
    """per callback the actions before it: 'ir', 'release', 'literal', 'bypass', ('L', n)"""
    for step, actions in enumerate(schedule):
        literal = bypass = False
        for act in actions:
            if act == "ir":
                ir = noise_ir(rng, ctx.num_samples, float(rng.uniform(300, 1200)), 0.05)
                ctx.set_impulse_response(s, ir)
                model.install(ir)
            elif act == "release":
                ctx.reverb_release(s)
                model.release()
            elif act == "literal":
                literal = True
            elif act == "bypass":
                bypass = True
            else:
                ctx.reverb_set_crossfade(s, act[1])
                model.set_crossfade(act[1])
        blk = noise_blocks(rng, 1, frame)[0]
        if bypass:                                       # touches neither the history nor the fade
            assert np.array_equal(ctx.reverb_process(s, blk, apply_reverb=False), blk)
            continue
        got = ctx.reverb_process(s, blk, literal_tail=literal)
        want = model.process(blk, literal=literal)
        assert close(got, want), (step, actions, np.abs(got - want).max())


CROSSFADE_SCHEDULES = {
    # L = the frame: the blocks before, during and after one change
    "one_frame": (64, [["ir"], [], ["ir"], [], ["ir"], []]),
    # a fade across callbacks, not a multiple of the frame; the literal tail during it; several installs between two callbacks
    "across_callbacks": (200, [["ir"], [], ["ir"], [], ["literal"], [], [], ["ir", "ir", "ir"], ["literal"], [], [], []]),
    # rule 3: a third IR at p0 = 128 of L = 320, then the new fade runs out
    "fold": (320, [["ir"], ["ir"], [], ["ir"], [], [], [], [], [], []]),
    # a new fade length in mid-fade ends the running fade at its target; the next one has the new length
    "set_crossfade_in_a_fade": (320, [["ir"], ["ir"], [], [("L", 100)], ["ir"], [], [], [("L", 0)], ["ir"], []]),
    "bypass_in_a_fade": (320, [["ir"], ["ir"], [], ["ir", "bypass"], [], ["bypass"], [], [], [], []]),
    "release_in_a_fade": (320, [["ir"], ["ir"], [], ["release"], [], ["ir"], [], ["release", "ir"], [], []]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CROSSFADE_SCHEDULES))
def test_crossfade_rules(pkg, name):
    L, schedule = CROSSFADE_SCHEDULES[name]
    ctx, (s,) = make_ctx(pkg, NS_X)
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_set_crossfade(s, L)                      # (before fs_reverb_init: both spectrum sets come from there)
    ctx.reverb_init(s, F_X)
    run_schedule(ctx, s, CrossfadeModel(NS_X, F_X, L), schedule, np.random.default_rng(len(name)))
    ctx.close()


@pytest.mark.gpu
def test_crossfade_enabled_after_init(pkg):
    """rule 4: the first callback after enabling takes the current IR unfaded (the second spectrum set comes from
    fs_reverb_set_crossfade here)"""
    ctx, (s,) = make_ctx(pkg, NS_X)
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_init(s, F_X)
    model = CrossfadeModel(NS_X, F_X, 0)
    schedule = [["ir"], [], ["ir", ("L", 200)], [], ["ir"], [], [], [], ["ir"], []]
    run_schedule(ctx, s, model, schedule, np.random.default_rng(8))
    ctx.close()


# One call or several: four partitioned sources, the first fading, the third bypassed in some callbacks, different IRs.
CALLS_B = 12


def drive_four(pkg, serve, engines=(PARTITIONED,) * 4):
    """serve(ctx, srcs, blocks [4][2F], apply [4]) -> what the test compares, per callback; the sources are driven alike"""
    ctx, srcs = make_ctx(pkg, NS_X, 4)
    rng = np.random.default_rng(66)
    for s, e in zip(srcs, engines):
        if e is not None:                                # (None: a source that never hears of the engine)
            ctx.reverb_set_engine(s, e)
        ctx.set_impulse_response(s, noise_ir(rng, NS_X, 600.0, 0.05))
    ctx.reverb_set_crossfade(srcs[0], 200)
    for s in srcs:
        ctx.reverb_init(s, F_X)
    res = []
    for c in range(CALLS_B):
        if c in (2, 3, 8):                               # the fading source: a fade, a fold one callback into it, another fade
            ctx.set_impulse_response(srcs[0], noise_ir(rng, NS_X, 600.0, 0.05))
        if c == 5:
            ctx.set_impulse_response(srcs[3], noise_ir(rng, NS_X, 600.0, 0.05))
        apply = [True, True, c not in (4, 5, 9), True]
        res.append(serve(ctx, srcs, noise_blocks(rng, 4, F_X), apply))
    ctx.close()
    return res


def serve_single(ctx, srcs, blk, apply):
    return np.stack([ctx.reverb_process(s, blk[i], apply_reverb=apply[i]) for i, s in enumerate(srcs)])


_single = {}


def single_calls(pkg):
    """[CALLS_B][4][2F]: the four partitioned sources served by single calls (computed once, read-only)"""
    if "out" not in _single:
        out = np.stack(drive_four(pkg, serve_single))
        out.setflags(write=False)
        _single["out"] = out
    return _single["out"]


@pytest.mark.gpu
def test_one_call_or_several_to_the_bit(pkg):
    single = single_calls(pkg)

    def serve(ctx, srcs, blk, apply):
        out, mix = ctx.reverb_process_batch(srcs, blk, apply=apply, want_out=True, want_mix=True)
        return out, mix

    both = drive_four(pkg, serve)
    only_mix = drive_four(pkg, lambda ctx, srcs, blk, apply: ctx.reverb_process_batch(srcs, blk, apply=apply, want_out=False, want_mix=True))
    assert np.abs(single).max() > 0.05
    for c in range(CALLS_B):
        out, mix = both[c]
        assert np.array_equal(out, single[c]), c
        want = out[0].copy()
        for r in range(1, 4):
            want = want + out[r]                          # fp32, list order
        assert np.array_equal(mix, want), c
        assert np.array_equal(np.asarray(only_mix[c]).reshape(-1), mix.reshape(-1)), c


@pytest.mark.gpu
def test_mixed_engines_in_one_batch(pkg):
    """[partitioned, direct, partitioned, direct] in one call: the partitioned rows are those of the single calls above, the
    direct rows those of a context whose sources never heard of the engine"""
    engines = (PARTITIONED, DIRECT, PARTITIONED, DIRECT)

    def serve(ctx, srcs, blk, apply):
        return ctx.reverb_process_batch(srcs, blk, apply=apply, want_out=True, want_mix=True)

    mixed = drive_four(pkg, serve, engines)
    single = single_calls(pkg)

    direct = np.stack(drive_four(pkg, serve_single, (None,) * 4))
    for c in range(CALLS_B):
        out, mix = mixed[c]
        for r in (0, 2):
            assert np.array_equal(out[r], single[c][r]), (c, r)
        for r in (1, 3):
            assert np.array_equal(out[r], direct[c][r]), (c, r)
        want = out[0].copy()
        for r in range(1, 4):
            want = want + out[r]
        assert np.array_equal(mix, want), c
    assert not np.array_equal(direct[-1][0], single[-1][0])   # (the engines differ in rounding: the rows were not all one engine)


@pytest.mark.gpu
def test_engine_switching(pkg):
    ns, frame = NS_X, F_X
    ctx, (a, b, c, d) = make_ctx(pkg, ns, 4)
    rng = np.random.default_rng(88)
    ir = noise_ir(rng, ns, 600.0, 0.05)
    for s in (a, b, c, d):
        ctx.set_impulse_response(s, ir)
    ctx.reverb_init(a, frame)
    ctx.reverb_init(b, frame)
    ctx.reverb_set_engine(a, PARTITIONED)               # recorded only: without a new fs_reverb_init nothing changes
    ctx.reverb_set_engine(c, PARTITIONED)
    ctx.reverb_init(c, frame)
    x = noise_blocks(rng, 8, frame)
    model = CrossfadeModel(ns, frame, 0)
    model.install(ir)
    for i in range(4):
        ya, yb, yc = (ctx.reverb_process(s, x[i]) for s in (a, b, c))
        assert np.array_equal(ya, yb), i
        assert close(yc, model.process(x[i])) and not np.array_equal(yc, yb), i   # (c does run the other engine)
    ctx.reverb_set_engine(c, DIRECT)                    # PARTITIONED -> init -> DIRECT -> init: a source that was always direct
    ctx.reverb_init(c, frame)
    ctx.reverb_init(d, frame)
    for i in range(4, 8):
        assert np.array_equal(ctx.reverb_process(c, x[i]), ctx.reverb_process(d, x[i])), i
    ctx.reverb_init(a, frame)                           # ... and a's recorded choice holds from its next init
    ctx.reverb_init(b, frame)
    model = CrossfadeModel(ns, frame, 0)
    model.install(ir)
    for i in range(4):
        ya, yb = ctx.reverb_process(a, x[i]), ctx.reverb_process(b, x[i])
        assert close(ya, model.process(x[i])) and not np.array_equal(ya, yb), i
    ctx.close()


@pytest.mark.gpu
def test_traced_irs_and_the_threads(pkg, scene_factory):
    """traced IRs through fs_update_sources: a partitioned callback after each tick against the published IR; then an audio
    thread of partitioned callbacks beside a game thread of reconstructs"""
    frame = 1024
    sc = scene_factory("starter_room", 4)
    ctx = pkg.Context(num_bands=4)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    s = ctx.create_source(sc.source)
    ctx.reverb_set_engine(s, PARTITIONED)
    ctx.reverb_init(s, frame)
    model = CrossfadeModel(ctx.num_samples, frame, 0)
    rng = np.random.default_rng(9)
    for tick in range(4):
        ctx.update_sources([s], traced_params(pkg, 300 + tick))
        ir = ctx.impulse_response(s, 0)
        assert ir.any()
        model.install(ir)
        for blk in noise_blocks(rng, 2, frame):         # the second callback takes nothing: its own spectra
            got, want = ctx.reverb_process(s, blk), model.process(blk)
            assert close(got, want), (tick, np.abs(got - want).max())

    done = threading.Event()
    errors, peak, count = [], [0.0], [0]

    def audio():
        arng = np.random.default_rng(60)
        try:
            while (not done.is_set() or count[0] < 20) and count[0] < 4000:
                y = ctx.reverb_process(s, noise_blocks(arng, 1, frame)[0])
                if not np.isfinite(y).all():
                    raise AssertionError(f"callback {count[0]}: a non-finite sample")
                peak[0] = max(peak[0], float(np.abs(y).max()))
                count[0] += 1
        except Exception as e:     # noqa: BLE001 — reported below
            errors.append(e)

    t = threading.Thread(target=audio)
    t.start()
    try:
        for tick in range(60):
            ctx.update_sources([s], traced_params(pkg, 1000 + tick, rays=4096))
    finally:
        done.set()
        t.join()
    assert not errors, errors
    assert count[0] >= 20 and 0.0 < peak[0] <= 1.0
    ctx.close()


@pytest.mark.gpu
def test_argument_checks(pkg):
    ctx, (s,) = make_ctx(pkg, NS_X)
    ir = noise_ir(np.random.default_rng(1), NS_X, 600.0, 0.05)
    ctx.set_impulse_response(s, ir)
    ctx.reverb_set_engine(s, PARTITIONED)
    for bad in (2, -1, 1 << 30):
        with pytest.raises(pkg.FrequenSeeError) as e:
            ctx.reverb_set_engine(s, bad)
        assert e.value.code == pkg._capi.ERR_INVALID_ARGUMENT
    with pytest.raises(pkg.FrequenSeeError) as e:
        ctx.reverb_set_engine(s + 17, PARTITIONED)
    assert e.value.code == pkg._capi.ERR_BAD_HANDLE
    with pytest.raises(pkg.FrequenSeeError):             # the refused calls left PARTITIONED in place: it refuses a frame of 15
        ctx.reverb_init(s, 15)
    ctx.reverb_set_engine(s, DIRECT)
    with pytest.raises(pkg.FrequenSeeError):
        ctx.reverb_set_engine(s, 2)
    ctx.reverb_init(s, 15)                              # ... and DIRECT, which takes it
    for ok in (DIRECT, PARTITIONED, DIRECT):
        ctx.reverb_set_engine(s, ok)
    ctx.close()
