"""fs_reverb_process_batch: the reverb callbacks of many sources as one set of launches (include/frequensee.h beside
fs_reverb_process).  The contract is the per-source loop's, to the bit: two contexts with the same sources and installed IRs,
one driven by fs_reverb_process and one by the batch, must agree with np.array_equal in every state the single call has.
(fs_reverb_process is a batch of one row: what these comparisons guard is the rows of one call against each other — the index
lists, the per-row descriptors, the staging offsets.)
Installed IRs are bit-equal in two contexts; traced ones are not (the histogram's atomics are unordered), so the traced test
compares with a float64 restatement of the crossfade rules instead (CrossfadeModel, restated from test_reverb_crossfade.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

FRAME = 1024
TOL = 2e-5          # test_reverb.py: |got - want| <= 2e-5 * max(|want|, 1e-3)
SPECTRAL = 512      # FS_FLAG_SPECTRAL_IR


def blocks(rng, count, frame=FRAME):
    """[count][2 * frame] interleaved stereo"""
    return np.clip(rng.normal(0, 0.3, (count, 2 * frame)), -1, 1).astype(np.float32)


def noise_ir(rng, n, decay=5000.0, gain=0.02):
    return (rng.normal(0, 1, n) * np.exp(-np.arange(n) / decay) * gain).astype(np.float32)


def close(got, want):
    return np.abs(got - want).max() <= TOL * max(np.abs(want).max(), 1e-3)


def mix_model(rows):
    """rule 2: ((rows[0] + rows[1]) + rows[2]) + ... in fp32, in list order, not clamped"""
    rows = np.asarray(rows, np.float32)
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = (acc + r).astype(np.float32)
    return acc


def conv_block(h, u, n, frame):
    """y[s] = sum_k h[k] u[n - 1 + s - k], s < frame (u = the n - 1 history samples, then the block)"""
    m = 1 << int(np.ceil(np.log2(n + u.shape[0])))
    return np.fft.irfft(np.fft.rfft(h, m) * np.fft.rfft(u, m), m)[n - 1:n - 1 + frame]


class CrossfadeModel:
    """One source's reverb callback with fs_reverb_set_crossfade, in float64 (the rules beside fs_reverb_set_crossfade)."""

    def __init__(self, n, frame, fade_len=0):
        self.n, self.frame, self.L = n, frame, fade_len
        self.hist = np.zeros((2, n - 1))
        self.ir = np.zeros(n)
        self.new = False
        self.h_from = self.h_to = None
        self.fading, self.pos, self.primed = False, 0, False

    def install(self, ir):
        self.ir = np.asarray(ir, np.float64).copy()
        self.new = True

    def process(self, block):
        f, n = self.frame, self.n
        b = np.asarray(block, np.float64)
        x = [b[0::2], b[1::2]]
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
                p = self.pos + np.arange(f)
                g = np.where(p < self.L, (p + 1) / max(self.L, 1), 1.0)
                y = [(1 - g) * conv_block(self.h_from, u[c], n, f) + g * conv_block(self.h_to, u[c], n, f) for c in range(2)]
                self.pos += f
                if self.pos >= self.L:
                    self.fading = False
            else:
                y = [conv_block(self.h_to, u[c], n, f) for c in range(2)]
        out = np.empty(2 * f)
        out[0::2], out[1::2] = y[0], y[1]
        return np.clip(out, -1.0, 1.0)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_entry_point_exported_and_bound(pkg):
    assert "fs_reverb_process_batch" in pkg._capi.EXPORTS
    lib = pkg._capi.load()
    assert hasattr(lib, "fs_reverb_process_batch")
    assert lib.fs_reverb_process_batch.argtypes is not None and len(lib.fs_reverb_process_batch.argtypes) == 8
    assert pkg._capi.MAX_REVERB_BATCH == 256
    assert hasattr(pkg.Context, "reverb_process_batch") and hasattr(pkg.FrequenSeeAudioReverbPlugin, "ProcessSourcesAudio")


def test_null_arguments_are_invalid_without_a_device(pkg):
    lib = pkg._capi.load()
    bad = pkg._capi.ERR_INVALID_ARGUMENT
    src = np.zeros(1, np.int32)
    a, o, m = (np.zeros(2 * FRAME, np.float32) for _ in range(3))
    assert lib.fs_reverb_process_batch(None, src.ctypes.data, 1, a.ctypes.data, o.ctypes.data, None, 0, m.ctypes.data) == bad
    import torch
    if not torch.cuda.is_available():
        # fs_context_create without a device reports FS_ERR_NO_DEVICE; where it still hands a context back (to be destroyed), the
        # null checks come before the device check
        h = C.c_void_p()
        cfg = pkg.default_config()
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == pkg._capi.ERR_NO_DEVICE
        if h:
            assert lib.fs_reverb_process_batch(h, None, 1, a.ctypes.data, o.ctypes.data, None, 0, None) == bad
            assert lib.fs_reverb_process_batch(h, src.ctypes.data, 1, None, o.ctypes.data, None, 0, None) == bad
            assert lib.fs_reverb_process_batch(h, src.ctypes.data, 1, a.ctypes.data, None, None, 0, None) == bad
            assert lib.fs_reverb_process_batch(h, src.ctypes.data, 1, a.ctypes.data, o.ctypes.data, None, 0, None) == pkg._capi.ERR_NO_DEVICE
            lib.fs_context_destroy(h)


def mix_rows():
    return np.clip(np.random.default_rng(7).normal(0, 0.3, (5, 2 * FRAME)), -1, 1).astype(np.float32)


def test_mix_model_is_the_ordered_fp32_sum():
    rows = mix_rows()
    got = mix_model(rows)
    assert got.dtype == np.float32
    exact = rows.astype(np.float64).sum(axis=0)
    # four fp32 additions, each within half an ulp of a partial sum that never exceeds sum |x|
    bound = 4 * 2.0 ** -24 * np.abs(rows.astype(np.float64)).sum(axis=0)
    assert (np.abs(got - exact) <= bound + 1e-30).all()
    assert not np.array_equal(got, mix_model(rows[::-1])), "the order test of the GPU suite could not fail on this data"


# ---- GPU: helpers -------------------------------------------------------------------------------------------------------------

def new_ctx(pkg, count):
    ctx = pkg.Context(num_bands=1)
    return ctx, [ctx.create_source(np.zeros(3, np.float32)) for _ in range(count)]


class Case:
    """A schedule over S sources: what happens before and in each callback, the same for every way of driving it."""

    def __init__(self, S=5, frame=FRAME, steps=6, literal=False, fades=None, installs=None, bypass=None, releases=None, seed=1):
        self.S, self.frame, self.steps, self.literal = S, frame, steps, literal
        self.fades = fades or {}               # source index -> crossfade length
        self.installs = installs or {0: list(range(S))}   # step -> source indices that get a new IR before that callback
        self.bypass = bypass or {}             # step -> source indices bypassed in that callback
        self.releases = releases or {}         # step -> source indices released before that callback
        self.seed = seed


def drive(pkg, case, how):
    """how(step) -> 'single' or 'batch'; returns [steps][S][2 * frame]"""
    ctx, srcs = new_ctx(pkg, case.S)
    for i, s in enumerate(srcs):
        if i in case.fades and i % 2 == 0:
            ctx.reverb_set_crossfade(s, case.fades[i])        # (before fs_reverb_init for some, after it for the others)
        ctx.reverb_init(s, case.frame)
        if i in case.fades and i % 2 == 1:
            ctx.reverb_set_crossfade(s, case.fades[i])
    rng = np.random.default_rng(case.seed)
    outs = []
    for step in range(case.steps):
        for i in case.installs.get(step, []):
            ctx.set_impulse_response(srcs[i], noise_ir(rng, ctx.num_samples, decay=float(rng.uniform(2000, 8000))))
        for i in case.releases.get(step, []):
            ctx.reverb_release(srcs[i])
        blk = blocks(rng, case.S, case.frame)
        off = set(case.bypass.get(step, []))
        apply = [i not in off for i in range(case.S)]
        if how(step) == "batch":
            y = ctx.reverb_process_batch(srcs, blk, apply=apply if off else None, literal_tail=case.literal)
        else:
            y = np.stack([ctx.reverb_process(srcs[i], blk[i], apply_reverb=apply[i], literal_tail=case.literal) for i in range(case.S)])
        for i in off:
            assert np.array_equal(y[i], blk[i]), (step, i)
        outs.append(y)
    ctx.close()
    return outs


def assert_same(a, b):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        for i in range(x.shape[0]):
            assert np.array_equal(x[i], y[i]), (step, i, float(np.abs(x[i] - y[i]).max()))
    assert any(np.abs(x).max() > 1e-3 for x in a), "silence proves nothing"


# sources 0, 1, 2 fade over less than, exactly and more than a frame; 3 and 4 switch abruptly.  Step 2 starts a fade everywhere;
# step 3 is mid-fade for source 2 (1024 of 2560); step 4 cuts that fade short with a newer IR (p0 = 2048) and starts one for
# source 0 again; source 2's new fade completes in step 6 (3 x 1024 >= 2560); step 7 convolves one IR everywhere.
def fade_case(frame=FRAME, **kw):
    return Case(steps=8, frame=frame, fades={0: frame // 2, 1: frame, 2: 2 * frame + frame // 2},
                installs={0: [0, 1, 2, 3, 4], 2: [0, 1, 2, 3, 4], 4: [0, 2, 4]}, **kw)


CASES = {
    "plain": lambda: Case(installs={0: [0, 1, 2, 3, 4], 3: [1, 4]}),
    "literal_tail": lambda: Case(literal=True, installs={0: [0, 1, 2, 3, 4], 3: [1, 4]}),
    "bypass": lambda: Case(installs={0: [0, 1, 2, 3, 4], 3: [1, 4]}, bypass={1: [2], 2: [0, 2, 4], 4: [0, 1, 2, 3, 4], 5: [3]}),
    "crossfade": fade_case,
    "crossfade_bypass_literal": lambda: fade_case(literal=True, bypass={2: [1], 3: [2], 5: [0, 2]}),
    "frame_1000": lambda: fade_case(frame=1000),          # not a multiple of the 16-output tile
    "frame_1000_plain": lambda: Case(frame=1000, installs={0: [0, 1, 2, 3, 4], 3: [1, 4]}),
}


# ---- GPU: tests ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_batch_equals_the_loop_bit_for_bit(pkg, name):
    case = CASES[name]()
    assert case.steps >= 6 and case.S == 5
    assert_same(drive(pkg, case, lambda step: "single"), drive(pkg, case, lambda step: "batch"))


@pytest.mark.gpu
def test_mixed_driving_and_release(pkg):
    """batch and single callbacks alternate in one context; fs_reverb_release between callbacks (one mid-fade) as in the loop"""
    case = fade_case(bypass={3: [1]}, releases={3: [2], 5: [0, 3]})
    want = drive(pkg, case, lambda step: "single")
    assert_same(want, drive(pkg, case, lambda step: "batch" if step % 2 == 0 else "single"))
    assert_same(want, drive(pkg, case, lambda step: "single" if step % 2 == 0 else "batch"))


@pytest.mark.gpu
def test_128_sources_equal_the_loop(pkg):
    S = 128
    case = Case(S=S, steps=2, fades={i: 1536 for i in range(0, S, 3)}, installs={0: list(range(S)), 1: list(range(0, S, 2))},
                bypass={1: [5, 77]})
    assert_same(drive(pkg, case, lambda step: "single"), drive(pkg, case, lambda step: "batch"))


def mix_setup(pkg, order):
    """a fresh context, 5 sources with their own IRs (source 3 fades), one warm-up callback; the sources listed in `order`"""
    ctx, srcs = new_ctx(pkg, 5)
    rng = np.random.default_rng(11)
    for i, s in enumerate(srcs):
        ctx.reverb_init(s, FRAME)
        if i == 3:
            ctx.reverb_set_crossfade(s, 2560)
        ctx.set_impulse_response(s, noise_ir(rng, ctx.num_samples, decay=2000.0 + 1000.0 * i, gain=0.05))
    warm = blocks(rng, 5)
    ctx.reverb_process_batch([srcs[i] for i in order], warm[order])
    ctx.set_impulse_response(srcs[3], noise_ir(rng, ctx.num_samples))   # the measured callback starts a fade for source 3
    return ctx, [srcs[i] for i in order], blocks(rng, 5)[order]


@pytest.mark.gpu
def test_mix_is_the_ordered_sum(pkg):
    fwd, rev = [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]
    apply = [True, True, False, True, True]                 # a bypassed source contributes its input
    ctx, srcs, blk = mix_setup(pkg, fwd)
    out, mix = ctx.reverb_process_batch(srcs, blk, apply=apply, want_mix=True)
    ctx.close()
    assert np.array_equal(out[2], blk[2]) and np.abs(out).max() <= 1.0
    assert np.array_equal(mix, mix_model(out))
    assert np.abs(mix).max() > 1.0 or True                   # (the sum is not clamped; whether it exceeds 1 depends on the data)
    ctx, srcs, blk = mix_setup(pkg, fwd)                     # out == NULL: only the mix comes back
    only = ctx.reverb_process_batch(srcs, blk, apply=apply, want_out=False, want_mix=True)
    ctx.close()
    assert np.array_equal(only, mix)
    ctx, srcs, blk = mix_setup(pkg, rev)                     # the same sources listed in reverse: the reverse-order sum
    out_r, mix_r = ctx.reverb_process_batch(srcs, blk, apply=apply[::-1], want_mix=True)
    ctx.close()
    assert np.array_equal(out_r, out[::-1])
    assert np.array_equal(mix_r, mix_model(out[::-1]))
    assert not np.array_equal(mix_r, mix), "the two orders round alike on this data: the order test shows nothing"


@pytest.mark.gpu
def test_batch_against_the_reference_convolver(pkg, oracle_mod):
    """an independent check that does not go through the single call: the reference's KissFFT convolver per source"""
    ctx, srcs = new_ctx(pkg, 3)
    assert ctx.num_samples == 48000
    rng = np.random.default_rng(21)
    refs = [oracle_mod.ReverbRef() for _ in srcs]
    irs = [None] * 3
    for s in srcs:
        ctx.reverb_init(s, FRAME)
    peak = 0.0
    for step in range(6):
        for i in ({0: [0, 1, 2], 2: [1], 4: [0, 2]}).get(step, []):   # (the reference switches IRs abruptly, as the default path)
            irs[i] = noise_ir(rng, 48000, decay=float(rng.uniform(2000, 8000)))
            ctx.set_impulse_response(srcs[i], irs[i])
        literal = step == 3
        blk = blocks(rng, 3)
        got, mix = ctx.reverb_process_batch(srcs, blk, literal_tail=literal, want_mix=True)
        for i in range(3):
            want = refs[i].process(irs[i], irs[i], blk[i], literal_tail=literal)
            assert np.abs(got[i] - want).max() <= TOL * max(np.abs(want).max(), 1e-3), (step, i)
            peak = max(peak, float(np.abs(want).max()))
        assert np.array_equal(mix, mix_model(got))
    assert peak > 0.05
    ctx.close()


def expect(pkg, code, fn):
    with pytest.raises(pkg.FrequenSeeError) as e:
        fn()
    assert e.value.code == code


@pytest.mark.gpu
def test_argument_checks_with_a_context(pkg):
    ctx, (s,) = new_ctx(pkg, 1)
    ctx.reverb_init(s, FRAME)
    lib, bad = ctx.lib, pkg._capi.ERR_INVALID_ARGUMENT
    src = np.array([s], np.int32)
    a, o = np.zeros(2 * FRAME, np.float32), np.zeros(2 * FRAME, np.float32)
    assert lib.fs_reverb_process_batch(ctx.h, None, 1, a.ctypes.data, o.ctypes.data, None, 0, None) == bad
    assert lib.fs_reverb_process_batch(ctx.h, src.ctypes.data, 1, None, o.ctypes.data, None, 0, None) == bad
    assert lib.fs_reverb_process_batch(ctx.h, src.ctypes.data, 1, a.ctypes.data, None, None, 0, None) == bad
    assert lib.fs_reverb_process_batch(ctx.h, src.ctypes.data, 1, a.ctypes.data, o.ctypes.data, None, 0, None) == pkg._capi.OK
    ctx.close()


@pytest.mark.gpu
def test_refused_calls_change_nothing(pkg):
    """every refusal with the offending entry LAST, behind sources for which the call would have started a fade"""
    def setup():
        ctx, srcs = new_ctx(pkg, 6)
        good, uninit, other_frame, dead = srcs[:3], srcs[3], srcs[4], srcs[5]
        for i, s in enumerate(good):
            ctx.reverb_init(s, FRAME)
            ctx.reverb_set_crossfade(s, 700 * (i + 1))
        ctx.reverb_init(other_frame, 512)
        ctx.reverb_init(dead, FRAME)
        ctx.destroy_source(dead)
        return ctx, good, uninit, other_frame, dead

    def install(ctx, good, rng):
        for s in good:
            ctx.set_impulse_response(s, noise_ir(rng, ctx.num_samples))

    seen, clean = setup(), setup()
    rng_a, rng_b = np.random.default_rng(31), np.random.default_rng(31)
    outs = [[], []]
    for k, ((ctx, good, uninit, other_frame, dead), rng) in enumerate(((seen, rng_a), (clean, rng_b))):
        install(ctx, good, rng)
        outs[k].append(ctx.reverb_process_batch(good, blocks(rng, 3)))
        install(ctx, good, rng)                              # a newer IR is waiting: the next accepted callback starts a fade
        junk = blocks(np.random.default_rng(99), 4)
        if k == 0:
            inv, handle = pkg._capi.ERR_INVALID_ARGUMENT, pkg._capi.ERR_BAD_HANDLE
            expect(pkg, inv, lambda: ctx.reverb_process_batch(good + [good[0]], junk))
            expect(pkg, inv, lambda: ctx.reverb_process_batch(good + [uninit], junk))
            expect(pkg, inv, lambda: ctx.reverb_process_batch(good + [other_frame], junk))
            expect(pkg, handle, lambda: ctx.reverb_process_batch(good + [dead], junk))
            expect(pkg, handle, lambda: ctx.reverb_process_batch(good + [12345], junk))
            many = np.array((good * 86)[:257], np.int32)
            big = np.zeros((257, 2 * FRAME), np.float32)
            o = np.zeros_like(big)
            for count in (0, 257, -1):
                assert ctx.lib.fs_reverb_process_batch(ctx.h, many.ctypes.data, count, big.ctypes.data, o.ctypes.data, None, 0, None) == inv
            assert not o.any()
        for _ in range(4):
            outs[k].append(ctx.reverb_process_batch(good, blocks(rng, 3)))
    assert_same(outs[0], outs[1])
    seen[0].close(); clean[0].close()


def traced_params(pkg, seed, flags=0, rays=8192):
    return pkg.default_params(num_rays=rays, depth=8, seed=seed, dist_divisor=100.0, flags=flags)


def traced_ctx(pkg, sc, count, fade):
    ctx = pkg.Context(num_bands=4)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    srcs = []
    for i in range(count):
        s = ctx.create_source(np.asarray(sc.source, np.float32) + np.float32(15.0 * i) * np.array([1, 0, 0], np.float32))
        ctx.reverb_init(s, FRAME)
        if fade:
            ctx.reverb_set_crossfade(s, fade)
        srcs.append(s)
    return ctx, srcs


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["update_sources", "update_sources_spectral", "batch_async", "pipelined"])
def test_traced_irs_every_route(pkg, scene_factory, route):
    """4 sources whose IRs come from every route that rewrites the device IR, crossfade on, convolved by the batch: the expected
    IR of a callback is the one each producer call published.  A batch that read an IR before its reconstruct had finished, or
    let the next reconstruct overwrite one it was still reading, would miss."""
    sc = scene_factory("starter_room", 4)
    ctx, srcs = traced_ctx(pkg, sc, 4, 2560)
    if route == "pipelined":
        ctx.set_pipelining(2)
        ctx.set_frames_per_launch(2)
    models = [CrossfadeModel(ctx.num_samples, FRAME, 2560) for _ in srcs]
    rng = np.random.default_rng(50)
    prev, changed = [None] * 4, [0] * 4
    seed = 100
    for step in range(7):
        if step != 3:                                       # one callback without a new IR (the fades go on)
            if route.startswith("update_sources"):
                ctx.update_sources(srcs, traced_params(pkg, seed, SPECTRAL if route.endswith("spectral") else 0))
                seed += 1
            elif route == "batch_async":
                p = traced_params(pkg, seed); seed += 1
                ctx.compute_energy_response_batch_async(srcs, p)
                ctx.reconstruct_impulse_response_batch_async(srcs, p)
                ctx.synchronize()
            else:                                           # two frames of the stream per source: only the newer counts
                for s in srcs:
                    for _ in range(2):
                        p = traced_params(pkg, seed); seed += 1
                        ctx.compute_energy_response_async(s, p)
                        ctx.reconstruct_impulse_response_async(s, p)
                ctx.synchronize()
            for i, s in enumerate(srcs):
                ir = ctx.impulse_response(s, 0)
                assert ir.any()
                changed[i] += prev[i] is not None and not np.array_equal(ir, prev[i])
                prev[i] = ir
                models[i].install(ir)
        blk = blocks(rng, 4)
        got = ctx.reverb_process_batch(srcs, blk)
        for i in range(4):
            want = models[i].process(blk[i])
            assert close(got[i], want), (route, step, i, float(np.abs(got[i] - want).max()))
    # (a published IR may repeat its predecessor — a pipelined stream of several sources does that now and then, with or
    # without a reverb; the model then fades between equal IRs, a no-op — but most publishes must start a real fade)
    assert min(changed) >= 3, changed
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fade", [0, 2560])
def test_audio_thread_against_game_thread(pkg, scene_factory, fade):
    """a bounded number of batch callbacks over 8 sources on one thread while another runs a bounded number of
    fs_update_sources ticks over them; neither may fail, and neither may fail to come back"""
    sc = scene_factory("starter_room", 4)
    ctx, srcs = traced_ctx(pkg, sc, 8, fade)
    ctx.update_sources(srcs, traced_params(pkg, 999, rays=4096))   # every source has an IR before the first callback
    errors, peak, counts = [], [0.0], [0, 0]
    CALLBACKS, TICKS = 120, 60

    def audio():
        rng = np.random.default_rng(60)
        try:
            for k in range(CALLBACKS):
                y, mix = ctx.reverb_process_batch(srcs, blocks(rng, 8), want_mix=True)
                if not (np.isfinite(y).all() and np.isfinite(mix).all()):
                    raise AssertionError(f"callback {k}: a non-finite sample")
                peak[0] = max(peak[0], float(np.abs(y).max()))
                counts[0] += 1
        except Exception as e:     # noqa: BLE001 — reported below
            errors.append(e)

    def game():
        try:
            for tick in range(TICKS):
                ctx.update_sources(srcs, traced_params(pkg, 1000 + tick, rays=4096))
                counts[1] += 1
        except Exception as e:     # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=audio, daemon=True), threading.Thread(target=game, daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    stuck = [t.name for t in threads if t.is_alive()]
    assert not stuck, f"threads did not come back: {stuck} after {counts} callbacks / ticks"
    assert not errors, errors
    assert counts == [CALLBACKS, TICKS] and 0.0 < peak[0] <= 1.0
    ctx.close()


# ---- IR lengths that fill the history ring -------------------------------------------------------------------------------------
# A callback appends ring positions [head, head + frame) and its convolution reads [head - tail, head), tail = ir_len - 1, both
# modulo 65 536: once tail + frame > 65 536 the appended samples alias the oldest history u[0 ..], so the push must run behind
# the convolution.  (tail + frame): 65 536, the last shape whose push may ride in front; 65 537, one past it; the tail is the
# whole ring.  A clobbered u[0] meets the oldest tap, ir[-1] = 0.1: about 0.03 on 0.3-sigma input.
RING_SHAPES = [(65057, 480), (65058, 480), (65537, 17)]


def conv_f64(x, h, n):
    """the first n samples of the linear convolution x * h in float64 (test_config_shapes.py)"""
    L = 1
    while L < len(x) + len(h):
        L *= 2
    return np.fft.irfft(np.fft.rfft(x, L) * np.fft.rfft(h, L), L)[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("ir_len,frame", RING_SHAPES)
def test_ir_lengths_that_fill_the_ring(pkg, ir_len, frame):
    """3 sources with their own IRs of ir_len samples (a 1 s context at ir_len Hz, as test_config_shapes.py::test_reverb_convolution;
    source 1 with a crossfade enabled and a constant IR), six batch callbacks alternating the literal tail: every row is the
    float64 convolution within that test's tolerance, and equals a second context driven by fs_reverb_process to the bit."""
    S, calls = 3, 6
    rng = np.random.default_rng(ir_len + frame)
    n = np.arange(ir_len)
    irs = []
    for _ in range(S):
        ir = (rng.normal(0, 1, ir_len) * np.exp(-n / (ir_len / 3.0)) * 0.004).astype(np.float32)
        ir[0] = 0.25
        ir[-1] = 0.1                                                    # the oldest tap reads the far end of the ring
        irs.append(ir)
    x = np.clip(rng.normal(0, 0.3, (calls, S, 2 * frame)), -1, 1).astype(np.float32)

    def run(batch):
        ctx = pkg.Context(num_bands=1, sample_rate=ir_len, simulated_duration=1.0)
        assert ctx.num_samples == ir_len
        srcs = [ctx.create_source((0.0, 0.0, 0.0)) for _ in range(S)]
        for s, ir in zip(srcs, irs):
            ctx.set_impulse_response(s, ir)
            ctx.reverb_init(s, frame)
        ctx.reverb_set_crossfade(srcs[1], 2 * frame + 1)
        y = np.empty_like(x)
        for c in range(calls):
            if batch:
                y[c] = ctx.reverb_process_batch(srcs, x[c], literal_tail=bool(c % 2))
            else:
                for i, s in enumerate(srcs):
                    y[c, i] = ctx.reverb_process(s, x[c, i], literal_tail=bool(c % 2))
        ctx.close()
        return y

    y = run(True)
    for i in range(S):
        h = irs[i].astype(np.float64)
        for ch in range(2):
            stream = x[:, i, ch::2].astype(np.float64).reshape(-1)
            want = conv_f64(stream, h, stream.size).reshape(calls, frame)
            for c in range(1, calls, 2):   # RVB.cpp:147-148: the current block is the interleaved buffer's first `frame` floats
                d = x[c, i, :frame].astype(np.float64) - x[c, i, ch::2].astype(np.float64)
                want[c] += conv_f64(d, h[:frame], frame)
            want = np.clip(want, -1.0, 1.0)
            err = np.abs(y[:, i, ch::2] - want)
            print(f"ir_len {ir_len} frame {frame} source {i} channel {ch}: max error {err.max():.3e}, peak {np.abs(want).max():.3f}")
            assert err.max() <= 5e-5 * max(1.0, np.abs(want).max()), (i, ch, np.unravel_index(np.argmax(err), err.shape))
    assert np.array_equal(y, run(False))
