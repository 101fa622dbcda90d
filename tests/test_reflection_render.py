"""fs_reflection_render_process_batch: the early reflections of every source of an audio callback — per source a bank of voices,
each the direct renderer's block (fractional slew-limited delay + band FIR) on one shared history, weighted by a ramping per-channel
gain and summed; voices are matched from callback to callback by a key and fade over one block when they appear or vanish
(include/frequensee.h, "early reflections on the audio thread").

The yardstick is Model below: a numpy float32 restatement of the header's rule, slot matching included, one history per source, a
Python loop over slots and taps, vectorised over the output sample.  It reads the band table from fs_direct_band_kernels, so the
device output must EQUAL it (tobytes()).  Beside it: the direct renderer's own yardstick and the direct renderer on the device (one
voice with gains (1, 1) is the direct sound), the same rule in float64 under a derived bound, known answers, the batch, state and
refusal rules.
"""
import ctypes as C

import numpy as np
import pytest

from test_direct_paths import device_free_bytes
from test_direct_render import EPS, F32, FS, Model as DirectModel
from test_direct_render import _close_contexts  # noqa: F401  (closes the contexts ctx_for caches when this module is done)
from test_direct_render import ctx_for, mix_model, noise, schedule, table_of, taps32
from test_reflection_paths import LIS, SRC, shoebox_world
from test_reverb_batch import noise_ir

MAX_VOICES = 32


def secs(samples, fs=FS):
    """the largest float32 time whose fp32 product with fs does not exceed `samples`: d1 = delay * (float)fs stays <= samples"""
    t = F32(samples / fs)
    while F32(t * F32(fs)) > F32(samples):
        t = np.nextafter(t, F32(0.0))
    return float(t)


# ---- without a GPU -----------------------------------------------------------------------------------------------------------
def test_struct_and_exports(pkg):
    cap = pkg._capi
    V, R = cap.ReflectionVoice, cap.ReflectionRenderRow
    assert C.sizeof(V) == 48 and C.sizeof(R) == 16
    assert (V.key.offset, V.delay.offset, V.band_gain.offset, V.channel_gain.offset) == (0, 4, 8, 40)
    assert (R.sounding.offset, R.started.offset, R.ended.offset, R.dropped.offset) == (0, 4, 8, 12)
    vd, rd = pkg.Context.REFLECTION_VOICE_DTYPE, pkg.Context.REFLECTION_RENDER_ROW_DTYPE
    assert vd.itemsize == 48 and rd.itemsize == 16
    assert [vd.fields[k][1] for k in ("key", "delay", "band_gain", "channel_gain")] == [0, 4, 8, 40]
    assert [rd.fields[k][1] for k in ("sounding", "started", "ended", "dropped")] == [0, 4, 8, 12]
    assert (cap.MAX_REFLECTION_VOICES, cap.MAX_REFLECTION_RENDER_BATCH) == (32, 256)
    for name in ("fs_reflection_render_init", "fs_reflection_render_release", "fs_reflection_render_process_batch"):
        assert name in cap.EXPORTS and hasattr(cap.load(), name)
    assert cap.load().fs_abi_version() == 5


def test_null_context_and_null_pointers(pkg):
    cap = pkg._capi
    lib = cap.load()
    src = (C.c_int32 * 1)(0)
    cnt = (C.c_int32 * 1)(1)
    blk = np.zeros(128, np.float32)
    out = np.full(128, 7.0, np.float32)
    mix = np.full(128, 7.0, np.float32)
    rows = np.full(4, 7, np.uint32)
    vo = np.zeros(1, dtype=pkg.Context.REFLECTION_VOICE_DTYPE)
    a, o, m, v, r = blk.ctypes.data, out.ctypes.data, mix.ctypes.data, vo.ctypes.data, rows.ctypes.data
    call = lib.fs_reflection_render_process_batch
    assert lib.fs_reflection_render_init(None, 0, 64, 15, 4, 0.01) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_reflection_render_release(None, 0) == cap.ERR_INVALID_ARGUMENT
    assert call(None, src, 1, a, v, cnt, 1, o, m, r) == cap.ERR_INVALID_ARGUMENT
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        cfg = cap.default_config(num_bands=1)
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == cap.ERR_NO_DEVICE and h
        try:
            assert lib.fs_reflection_render_init(h, 0, 64, 15, 4, 0.01) == cap.ERR_NO_DEVICE
            assert b"no CPU fallback" in lib.fs_last_error(h)
            assert call(h, src, 1, a, v, cnt, 1, o, m, r) == cap.ERR_NO_DEVICE
            assert call(h, None, 1, a, v, cnt, 1, o, m, r) == cap.ERR_INVALID_ARGUMENT
            assert call(h, src, 1, None, v, cnt, 1, o, m, r) == cap.ERR_INVALID_ARGUMENT
            assert call(h, src, 1, a, None, cnt, 1, o, m, r) == cap.ERR_INVALID_ARGUMENT
            assert call(h, src, 1, a, v, None, 1, o, m, r) == cap.ERR_INVALID_ARGUMENT
            assert call(h, src, 1, a, v, cnt, 1, None, None, r) == cap.ERR_INVALID_ARGUMENT
        finally:
            lib.fs_context_destroy(h)
    assert np.all(out == 7.0) and np.all(mix == 7.0) and np.all(rows == 7)


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
class Model:
    """One source's callback, as include/frequensee.h states it.  An entry is (key, delay in s, band gains, channel gains).
    process() returns (the fp32 output [F * 2], the row's counts (sounding, started, ended, dropped)); with want64 also the same
    rule with d, i, f, a from the fp32 rule and every multiply-accumulate in float64, and the bound's sum over the sounding slots
    of max(|w0|, |w1|) max(sum|c0|, sum|c1|)."""

    def __init__(self, table, frame, voices, fs=FS):
        self.k = np.asarray(table, np.float32)
        self.B, self.T = self.k.shape
        self.F, self.V, self.fs = frame, voices, fs
        self.release()

    def release(self):
        self.x = [np.zeros(0, np.float32), np.zeros(0, np.float32)]   # x(n) for n >= 0; zero before
        self.n0 = 0
        self.slots = [None] * self.V   # None = free, else dict(key, d0, g0, w0)

    def sample(self, ch, p):
        x = self.x[ch]
        return np.where(p >= 0, x[np.maximum(p, 0)], F32(0.0)).astype(np.float32)

    def match(self, entries):
        """rule 1: per slot None or (kind, d0, g0, w0, d1, g1, w1, key), and the counts"""
        plan = [None] * self.V
        started = ended = dropped = 0
        target = {}
        for key, delay, gains, chan in entries:
            assert key not in target
            target[key] = (F32(delay) * F32(self.fs), np.asarray(gains, np.float32)[:self.B].copy(), np.asarray(chan, np.float32).copy())
        zero2 = np.zeros(2, np.float32)
        free = [j for j in range(self.V) if self.slots[j] is None]   # as the callback began
        for j, st in enumerate(self.slots):
            if st is None:
                continue
            if st["key"] in target:
                d1, g1, w1 = target.pop(st["key"])
                plan[j] = ("continue", st["d0"], st["g0"], st["w0"], d1, g1, w1, st["key"])
            else:
                plan[j] = ("end", st["d0"], st["g0"], st["w0"], st["d0"], st["g0"], zero2, st["key"])
                ended += 1
        for key, (d1, g1, w1) in target.items():   # (a dict keeps the list order)
            if free:
                plan[free.pop(0)] = ("start", d1, g1, zero2, d1, g1, w1, key)
                started += 1
            else:
                dropped += 1
        return plan, (sum(p is not None for p in plan), started, ended, dropped)

    def process(self, block, entries, want64=False):
        F, T = self.F, self.T
        block = np.asarray(block, np.float32)
        plan, row = self.match(entries)
        half = F32(0.5) * F32(F)
        s = np.arange(F)
        a = (s + 1).astype(np.float32) / F32(F)
        a64 = a.astype(np.float64)
        for ch in range(2):
            self.x[ch] = np.concatenate([self.x[ch], block[ch::2]])
        out = np.zeros(2 * F, np.float32)
        out64 = np.zeros(2 * F, np.float64)
        weight = 0.0
        for j, p in enumerate(plan):   # ascending slot number
            if p is None:
                continue
            kind, d0, g0, w0, d1, g1, w1, key = p
            e = np.clip(d1 - d0, -half, half).astype(np.float32)
            c0, c1 = taps32(self.k, g0), taps32(self.k, g1)
            dc = c1 - c0
            d = d0 + a * e
            fl = np.floor(d)
            f = d - fl
            i = fl.astype(np.int64)
            assert a.dtype == d.dtype == f.dtype == dc.dtype == np.float32
            for ch in range(2):
                acc = [np.zeros(F, np.float32) for _ in range(4)]
                acc64 = np.zeros(F, np.float64)
                for t in range(T):
                    c = c0[t] + a * dc[t]
                    q = self.n0 + s - t - i
                    xp, xm = self.sample(ch, q), self.sample(ch, q - 1)
                    v = xp + f * (xm - xp)
                    acc[t % 4] = acc[t % 4] + c * v
                    if want64:
                        c64 = np.float64(c0[t]) + a64 * (np.float64(c1[t]) - np.float64(c0[t]))
                        acc64 += c64 * (xp.astype(np.float64) + f.astype(np.float64) * (xm.astype(np.float64) - xp.astype(np.float64)))
                y = (acc[0] + acc[1]) + (acc[2] + acc[3])
                dw = w1[ch] - w0[ch]
                w = w0[ch] + a * dw
                assert y.dtype == w.dtype == np.float32
                out[ch::2] = out[ch::2] + w * y
                out64[ch::2] += (np.float64(w0[ch]) + a64 * (np.float64(w1[ch]) - np.float64(w0[ch]))) * acc64
            csum = max(np.abs(c0.astype(np.float64)).sum(), np.abs(c1.astype(np.float64)).sum())
            weight += float(max(np.abs(w0).max(), np.abs(w1).max())) * csum
            if kind == "end":
                self.slots[j] = None
            else:
                g_after = np.zeros(self.B, np.float32)
                g_after[:] = g1
                self.slots[j] = dict(key=key, d0=F32(d0 + e), g0=g_after, w0=w1.copy())
        assert out.dtype == np.float32
        self.n0 += F
        if want64:
            return out, row, out64, weight
        return out, row


def entry(key, samples, gains, chan, fs=FS):
    return (key, secs(samples, fs), np.asarray(gains, np.float32), np.asarray(chan, np.float32))


def test_model_equals_the_direct_yardstick(pkg):
    """one voice with constant channel gains (1, 1) IS the direct sound: from the second callback on (the first is the fade-in) the
    two yardsticks give the same values, through the direct renderer's own schedule (ramps, new gains, a slew-limited jump)"""
    for bands, frame, taps in ((3, 64, 15), (8, 320, 63)):
        table = pkg.Context.direct_band_kernels(FS, bands, taps)
        m, d = Model(table, frame, 2), DirectModel(table, frame)
        rng = np.random.default_rng(31 + taps)
        for cb, (delay, gains) in enumerate(schedule(frame, bands, rng)):
            blk = noise(rng, 1, frame)[0]
            got, row = m.process(blk, [(7, delay, gains, (1.0, 1.0))])
            want = d.process(blk, delay, gains)
            assert row == (1, 1 if cb == 0 else 0, 0, 0)
            if cb:
                assert np.array_equal(got, want), f"callback {cb + 1}"
                assert got.any()


def test_restatement_against_float64(pkg):
    """|y - y64| <= (T + 8 + K + 2) 2^-24 max|x| sum_j max(|w0_j|, |w1_j|) max(sum|c0_j|, sum|c1_j|): the direct renderer's derived
    per-voice bound (T rounded products and sums plus the lerp and tap interpolation) plus one rounding per product and per sum of
    rule 3 (and the gain ramp's two); derived, not measured.  60 random cases, K <= 4 voices, the second callback ramping"""
    rng = np.random.default_rng(0xEA21)
    worst = 0.0
    for case in range(60):
        bands, taps, frame, K = int(rng.choice([1, 3, 8])), int(rng.choice([15, 63, 255])), 32, int(rng.integers(1, 5))
        m = Model(pkg.Context.direct_band_kernels(FS, bands, taps), frame, K)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            entries = [(k, float(rng.uniform(0.0, 300.0)) / FS, rng.uniform(0.0, 1.0, 8), rng.uniform(-1.0, 1.0, 2)) for k in range(K)]
            y, row, y64, weight = m.process(blk, entries, want64=True)
        assert row == (K, 0, 0, 0)
        bound = (taps + 8 + K + 2) * EPS * 1.0 * weight
        worst = max(worst, float(np.abs(y - y64).max() / bound))
    print(f"restatement vs float64: worst share of the bound {worst:.3f}")
    assert worst <= 1.0


class _Ctx:   # what Voices() reads of a context
    class cfg:
        sample_rate = FS


def _paths(pkg, n):
    return np.zeros(n, dtype=pkg.Context.REFLECTION_DTYPE), np.zeros(1, dtype=pkg.Context.REFLECTION_ROW_DTYPE)[0]


def test_voices_known_answers(pkg):
    plug = pkg.FrequenSeeAudioReflectionPlugin.__new__(pkg.FrequenSeeAudioReflectionPlugin)
    plug.ctx, plug.Taps = _Ctx, 255
    paths, row = _paths(pkg, 4)
    right = np.array([0.0, 1.0, 0.0])
    paths["direction"] = [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]]
    paths["triangle"] = [11, 5, 2, 99]
    paths["delay"] = [0.01, 0.001, 0.02, 0.03]   # 0.001 s is less than the latency of 127 samples
    paths["length"] = [200.0, 50.0, 400.0, 800.0]
    paths["reflectance"] = np.arange(32, dtype=np.float32).reshape(4, 8) / 32
    row["returned"] = 3
    v = plug.Voices(row, paths, right=right)
    assert v.dtype == pkg.Context.REFLECTION_VOICE_DTYPE and v.shape == (3,), "only the returned paths become entries"
    assert list(v["key"]) == [11, 5, 2]
    assert np.array_equal(v["band_gain"], paths["reflectance"][:3])
    latency = 127 / FS
    assert v["delay"][0] == F32(float(F32(0.01)) - latency) and v["delay"][1] == 0.0 and v["delay"][2] == F32(float(F32(0.02)) - latency)
    r2 = np.sqrt(0.5)
    assert np.abs(v["channel_gain"] - [[0.0, 1.0], [r2, r2], [1.0, 0.0]]).max() <= 1e-7
    flat = plug.Voices(row, paths)
    assert np.array_equal(flat["channel_gain"], np.ones((3, 2), np.float32))
    near = plug.Voices(row, paths, right=right, reference_length=100.0)   # min(1, 100 / length) = 0.5, 1, 0.25
    assert np.abs(near["channel_gain"] - np.array([[0.0, 0.5], [r2, r2], [0.25, 0.0]])).max() <= 1e-7
    row["returned"] = 0
    assert plug.Voices(row, paths).shape == (0,)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def one(ctx, src, block, entries, **kw):
    out, rows = ctx.reflection_render_process_batch([src], block[None], [entries], **kw)
    return out[0], tuple(int(x) for x in rows[0])


def assert_same(got, want, where):
    (g, grow), (w, wrow) = got, want
    assert grow == wrow, f"{where}: rows {grow} != {wrow}"
    bad = np.nonzero(g != w)[0]
    assert g.tobytes() == w.tobytes(), f"{where}: {bad.size} samples differ, first at {bad[:4]}: {g[bad[:4]]} != {w[bad[:4]]}"


def bank_schedule(rng):
    """eight callbacks on three slots: two keys start | unchanged | fractional delays up and down, new band and channel gains, one
    negative | key 20 vanishes and 30 starts (on the free slot 2, not the ending slot 1) | 20 returns, the list permuted | four
    entries and no slot left for the last | empty: all end | empty: silence — (entries, the row's counts)"""
    g = [rng.uniform(0.0, 1.0, 8).astype(np.float32) for _ in range(6)]
    w = [rng.uniform(0.2, 1.0, 2).astype(np.float32) for _ in range(6)]
    neg = np.array([-0.6, 0.4], np.float32)
    return [
        ([entry(10, 100.25, g[0], w[0]), entry(20, 131.5, g[1], w[1])], (2, 2, 0, 0)),
        ([entry(10, 100.25, g[0], w[0]), entry(20, 131.5, g[1], w[1])], (2, 0, 0, 0)),
        ([entry(10, 110.6, g[2], neg), entry(20, 120.3, g[3], w[3])], (2, 0, 0, 0)),
        ([entry(10, 110.6, g[2], neg), entry(30, 77.75, g[4], w[4])], (3, 1, 1, 0)),
        ([entry(20, 140.0, g[1], w[1]), entry(30, 80.5, g[4], w[4]), entry(10, 105.1, g[2], w[2])], (3, 1, 0, 0)),
        ([entry(10, 105.1, g[2], w[2]), entry(20, 140.0, g[1], w[1]), entry(30, 80.5, g[4], w[4]), entry(40, 50.0, g[5], w[5])], (3, 0, 0, 1)),
        ([], (3, 0, 3, 0)),
        ([], (0, 0, 0, 0)),
    ]


# F = 64: a partial tile; 256: exactly one tile; 320: a full tile and a partial one.  T = 5, 9: one tail step behind one and two full
# groups of four (T = 1 never enters the four-wide loop, the other lengths are 3 mod 4)
SHAPES = [(64, 1), (64, 15), (64, 255), (320, 15), (320, 255), (64, 5), (320, 9), (256, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("bands", [1, 3, 8])
@pytest.mark.parametrize("frame,taps", SHAPES)
def test_bit_equal_to_the_restatement(pkg, bands, frame, taps):
    ctx = ctx_for(pkg, bands)
    src = ctx.create_source()
    ctx.reflection_render_init(src, frame, taps, 3, 0.02)
    m = Model(table_of(pkg, ctx, taps), frame, 3)
    rng = np.random.default_rng(1000 * bands + frame + taps)
    for cb, (entries, counts) in enumerate(bank_schedule(rng)):
        blk = noise(rng, 1, frame)[0]
        want = m.process(blk, entries)
        assert want[1] == counts, f"callback {cb + 1}: the yardstick's own counts"
        got = one(ctx, src, blk, entries)
        assert_same(got, want, f"callback {cb + 1}")
        if cb == 3:
            assert [None if s is None else s["key"] for s in m.slots] == [10, None, 30]
        if cb == 7:
            assert not got[0].any(), "a row without a sounding slot is exactly zero"
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_longest_filter(pkg):
    ctx = ctx_for(pkg, 8)
    src = ctx.create_source()
    frame, taps = 64, 2047
    ctx.reflection_render_init(src, frame, taps, 2, 0.02)
    m = Model(table_of(pkg, ctx, taps), frame, 2)
    rng = np.random.default_rng(2047)
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    for cb, (da, db) in enumerate(((300.5, 10.0), (310.25, 4.75), (310.25, 40.0))):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(1, da, g[0], (0.9, -0.3)), entry(2, db, g[1], (0.2, 0.7))]
        assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_one_voice_is_the_direct_renderer(pkg):
    """source A: one voice with gains (1, 1); source B: fs_direct_render_process_batch; the same input and targets.  From the second
    callback on (the first fades in) the outputs are equal by value"""
    ctx = ctx_for(pkg, 3)
    frame, taps = 320, 15
    a, b = ctx.create_source(), ctx.create_source()
    ctx.reflection_render_init(a, frame, taps, 2, 0.02)
    ctx.direct_render_init(b, frame, taps, 0.02)
    rng = np.random.default_rng(8)
    for cb, (delay, gains) in enumerate(schedule(frame, 3, rng)):
        blk = noise(rng, 1, frame)[0]
        got, row = one(ctx, a, blk, [(5, delay, gains, (1.0, 1.0))])
        want = ctx.direct_render_process_batch([b], blk[None], [(delay, gains)])[0]
        assert row == (1, 1 if cb == 0 else 0, 0, 0)
        if cb:
            assert np.array_equal(got, want), f"callback {cb + 1}"
    ctx.destroy_source(a)
    ctx.destroy_source(b)


@pytest.mark.gpu
def test_five_steady_voices_are_five_direct_sources(pkg):
    """delays from 0 to D, distinct gains: the bank's output is acc = acc + w_j * y_j (fp32, slot order) over the outputs y_j of five
    direct sources fed the same input"""
    ctx = ctx_for(pkg, 3)
    frame, taps, D = 64, 15, 480
    bank = ctx.create_source()
    ctx.reflection_render_init(bank, frame, taps, 5, D / FS)
    direct = [ctx.create_source() for _ in range(5)]
    for s in direct:
        ctx.direct_render_init(s, frame, taps, D / FS)
    rng = np.random.default_rng(55)
    delays = [secs(x) for x in (0.0, 120.25, 240.5, 360.75, float(D))]
    assert D - 1e-3 < F32(delays[4]) * F32(FS) <= D
    gains = rng.uniform(0, 1, (5, 8)).astype(np.float32)
    chan = rng.uniform(-1, 1, (5, 2)).astype(np.float32)
    for cb in range(4):
        blk = noise(rng, 1, frame)[0]
        got, row = one(ctx, bank, blk, [(100 + j, delays[j], gains[j], chan[j]) for j in range(5)])
        ys = ctx.direct_render_process_batch(direct, np.repeat(blk[None], 5, 0), [(delays[j], gains[j]) for j in range(5)])
        acc = np.zeros(2 * frame, np.float32)
        for j in range(5):
            for ch in range(2):
                acc[ch::2] = acc[ch::2] + chan[j][ch] * ys[j][ch::2]
        assert row == (5, 5 if cb == 0 else 0, 0, 0)
        if cb:
            assert np.array_equal(got, acc), f"callback {cb + 1}"
    for s in direct + [bank]:
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_full_bank(pkg):
    ctx = ctx_for(pkg, 3)
    frame, taps = 64, 15
    src = ctx.create_source()
    ctx.reflection_render_init(src, frame, taps, MAX_VOICES, 0.02)
    m = Model(table_of(pkg, ctx, taps), frame, MAX_VOICES)
    rng = np.random.default_rng(32)
    for cb in range(3):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(1000 + k, rng.uniform(0, 900), rng.uniform(0, 1, 8), rng.uniform(-1, 1, 2)) for k in range(MAX_VOICES)]
        got = one(ctx, src, blk, entries)
        assert got[1] == (32, 32 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_batch_single_and_permuted_agree(pkg):
    """sources of 1, 3 and 8 slots with 0, 1 and 5 entries (rotating) in one batch of stride 5"""
    ctx = ctx_for(pkg, 3)
    frame, taps, n = 320, 15, 3
    V = [1, 3, 8]
    sets = [[ctx.create_source() for _ in range(n)] for _ in range(3)]   # one call | three calls | permuted order
    for group in sets:
        for s, v in zip(group, V):
            ctx.reflection_render_init(s, frame, taps, v, 0.02)
    models = [Model(table_of(pkg, ctx, taps), frame, v) for v in V]
    rng = np.random.default_rng(3)
    perm = [2, 0, 1]
    counts = [[0, 1, 5], [1, 5, 0], [5, 0, 1], [1, 1, 5]]
    for cb in range(4):
        blk = noise(rng, n, frame)
        lists = [[entry(50 + k, rng.uniform(0, 600), rng.uniform(0, 1, 8), rng.uniform(-1, 1, 2)) for k in range(counts[cb][i])] for i in range(n)]
        out, mix, rows = ctx.reflection_render_process_batch(sets[0], blk, lists, stride=5, want_mix=True)
        singles = [one(ctx, sets[1][i], blk[i], lists[i], stride=5) for i in range(n)]
        pout, pmix, prows = ctx.reflection_render_process_batch([sets[2][i] for i in perm], blk[perm], [lists[i] for i in perm], stride=5,
                                                                want_mix=True)
        for i in range(n):
            want = models[i].process(blk[i], lists[i])
            assert_same((out[i], tuple(int(x) for x in rows[i])), want, f"batch {cb} {i}")
            assert_same(singles[i], want, f"single {cb} {i}")
            j = perm.index(i)
            assert_same((pout[j], tuple(int(x) for x in prows[j])), want, f"permuted {cb} {i}")
        assert mix.tobytes() == mix_model(out).tobytes(), "mix is not the fp32 sum in list order"
        assert pmix.tobytes() == mix_model(pout).tobytes()
    assert tuple(int(x) for x in rows[0]) == (1, 0, 0, 0) and models[0].slots[0] is not None
    blk2 = noise(rng, n, frame)   # with out == NULL only the mix comes back; the state moves on all the same
    only_mix, rows2 = ctx.reflection_render_process_batch(sets[0], blk2, lists, stride=5, want_out=False, want_mix=True)
    wants = [models[i].process(blk2[i], lists[i]) for i in range(n)]
    assert only_mix.shape == (2 * frame,) and only_mix.tobytes() == mix_model([w[0] for w in wants]).tobytes()
    assert [tuple(int(x) for x in r) for r in rows2] == [w[1] for w in wants]
    for s in sum(sets, []):
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_ring_wrap(pkg):
    """max delay 400 samples, T = 255, F = 320: the ring is 1024 floats, and twenty callbacks write 6400"""
    ctx = ctx_for(pkg, 3)
    src = ctx.create_source()
    frame, taps = 320, 255
    ctx.reflection_render_init(src, frame, taps, 3, 400.0 / FS)
    m = Model(table_of(pkg, ctx, taps), frame, 3)
    rng = np.random.default_rng(1024)
    for cb in range(20):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(k, x, rng.uniform(0, 1, 8), rng.uniform(-1, 1, 2)) for k, x in ((1, 400.0), (2, rng.uniform(0, 400)))]
        if cb % 5 == 4:
            entries = entries[:1]   # the second voice ends, and starts again in the next callback
        assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    cap = pkg._capi
    lib = cap.load()
    ctx = ctx_for(pkg, 3)
    frame, taps = 64, 15
    srcs = [ctx.create_source() for _ in range(3)]
    for s, v in zip(srcs, (2, 3, 4)):
        ctx.reflection_render_init(s, frame, taps, v, 0.01)   # D = 480
    other_frame, other_taps, uninit, dead = (ctx.create_source() for _ in range(4))
    ctx.reflection_render_init(other_frame, 128, taps, 3, 0.01)
    ctx.reflection_render_init(other_taps, frame, 31, 3, 0.01)
    ctx.reflection_render_init(dead, frame, taps, 3, 0.01)
    ctx.destroy_source(dead)
    models = [Model(table_of(pkg, ctx, taps), frame, v) for v in (2, 3, 4)]
    rng = np.random.default_rng(5)
    gains = np.full(8, 0.5, np.float32)

    def good_call():
        blk = noise(rng, 3, frame)
        lists = [[entry(k, rng.uniform(0, 400), gains, (0.5, 0.25)) for k in range(2)] for _ in range(3)]
        out, rows = ctx.reflection_render_process_batch(srcs, blk, lists)
        for i in range(3):
            assert_same((out[i], tuple(int(x) for x in rows[i])), models[i].process(blk[i], lists[i]), f"source {i}")

    good_call()
    blk = noise(rng, 3, frame)
    sentinel = np.full((3, 2 * frame), 7.0, np.float32)
    out, mix = sentinel.copy(), sentinel[0].copy()
    rows = np.full((3, 4), 7, np.uint32)
    inf, nan = float("inf"), float("nan")
    base = np.zeros((3, 2), dtype=pkg.Context.REFLECTION_VOICE_DTYPE)
    for i in range(3):
        for e in range(2):
            base[i, e] = (e, 0.001 * (i + e + 1), gains, (0.5, 0.25))

    def call(sources=srcs, count=3, table=base, counts=(2, 2, 2), stride=2, blocks=blk, dest=out, mixed=None, voices=True, cnts=True, handles=True):
        arr = (C.c_int32 * len(sources))(*sources)
        t = np.ascontiguousarray(table)
        n = np.asarray(counts, np.int32)
        return lib.fs_reflection_render_process_batch(ctx.h, arr if handles else None, count, blocks.ctypes.data if blocks is not None else None,
                                                      t.ctypes.data if voices else None, n.ctypes.data if cnts else None, stride,
                                                      dest.ctypes.data if dest is not None else None,
                                                      mixed.ctypes.data if mixed is not None else None, rows.ctypes.data)

    def with_entry(field, value, index=None):
        t = base.copy()
        if index is None:
            t[1, 1][field] = value
        else:
            t[1, 1][field][index] = value
        return t

    for counts in ((2, 3, 2), (2, -1, 2)):
        assert call(counts=counts) == cap.ERR_INVALID_ARGUMENT, counts
    wide = np.zeros((3, 33), dtype=pkg.Context.REFLECTION_VOICE_DTYPE)
    for stride, table in ((0, base), (-1, base), (33, wide)):
        assert call(stride=stride, table=table, counts=(0, 0, 0)) == cap.ERR_INVALID_ARGUMENT, stride
    assert call(table=with_entry("key", 0)) == cap.ERR_INVALID_ARGUMENT, "a key twice in one row"
    for v in (-0.001, nan, inf, 481.0 / FS):
        assert call(table=with_entry("delay", v)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (-0.5, nan, inf):
        assert call(table=with_entry("band_gain", v, 1)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (nan, inf, -inf):
        assert call(table=with_entry("channel_gain", v, 1)) == cap.ERR_INVALID_ARGUMENT, v
    for count in (0, -1, 257):
        assert call(count=count) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], srcs[1], srcs[0]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_frame, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_taps, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], uninit, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], dead, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[srcs[0], 12345, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[-1, srcs[1], srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(handles=False) == cap.ERR_INVALID_ARGUMENT
    assert call(blocks=None) == cap.ERR_INVALID_ARGUMENT
    assert call(voices=False) == cap.ERR_INVALID_ARGUMENT
    assert call(cnts=False) == cap.ERR_INVALID_ARGUMENT
    assert call(dest=None) == cap.ERR_INVALID_ARGUMENT, "out == NULL && mix == NULL"
    assert call(table=with_entry("delay", nan), mixed=mix) == cap.ERR_INVALID_ARGUMENT
    assert np.array_equal(out, sentinel) and np.array_equal(mix, sentinel[0]) and np.all(rows == 7), "a refused call wrote"
    good_call()   # every refused call left all three sources as they were
    blk = noise(rng, 3, frame)
    assert call(table=with_entry("band_gain", nan, 3), blocks=blk) == cap.OK, "entries beyond num_bands are ignored"
    for i in range(3):   # (that call was a callback like any other)
        lst = [(int(base[i, e]["key"]), float(base[i, e]["delay"]), gains, (0.5, 0.25)) for e in range(2)]
        assert_same((out[i], tuple(int(x) for x in rows[i])), models[i].process(blk[i], lst), f"source {i}")

    # init refusals; a refused init leaves the source as it was
    for args in ((15, 15, 3, 0.01), (16385, 15, 3, 0.01), (frame, 16, 3, 0.01), (frame, 0, 3, 0.01), (frame, 2049, 3, 0.01),
                 (frame, taps, 0, 0.01), (frame, taps, -1, 0.01), (frame, taps, 33, 0.01), (frame, taps, 3, -0.01), (frame, taps, 3, nan),
                 (frame, taps, 3, inf), (frame, taps, 3, 22.0)):
        assert lib.fs_reflection_render_init(ctx.h, srcs[0], args[0], args[1], args[2], C.c_float(args[3])) == cap.ERR_INVALID_ARGUMENT, args
    assert lib.fs_reflection_render_init(ctx.h, 12345, frame, taps, 3, C.c_float(0.01)) == cap.ERR_BAD_HANDLE
    assert lib.fs_reflection_render_release(ctx.h, 12345) == cap.ERR_BAD_HANDLE
    assert lib.fs_reflection_render_release(ctx.h, uninit) == cap.OK
    good_call()
    for s in srcs + [other_frame, other_taps, uninit]:
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_release_and_reinit(pkg):
    ctx = ctx_for(pkg, 3)
    src = ctx.create_source()
    rng = np.random.default_rng(8)
    frame, taps, V = 64, 15, 3
    ctx.reflection_render_init(src, frame, taps, V, 0.02)
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    entries = [entry(1, 50.5, g[0], (1.0, 0.5)), entry(2, 300.0, g[1], (0.5, 1.0))]
    for _ in range(2):
        one(ctx, src, noise(rng, 1, frame)[0], entries)
    ctx.reflection_render_release(src)   # zero history, every slot free: the same keys fade in from silence
    m = Model(table_of(pkg, ctx, taps), frame, V)
    for cb in range(2):
        blk = noise(rng, 1, frame)[0]
        got = one(ctx, src, blk, entries)
        assert got[1] == (2, 2 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"after release, callback {cb + 1}")
    for frame, taps, V in ((320, 15, 1), (64, 255, 5)):   # another F, another T, another V — with voices held
        ctx.reflection_render_init(src, frame, taps, V, 0.02)
        m = Model(table_of(pkg, ctx, taps), frame, V)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"{(frame, taps, V)} callback {cb + 1}")
    ctx.destroy_source(src)   # with voices held
    other = ctx.create_source()
    ctx.reflection_render_init(other, 64, 15, 2, 0.02)
    m = Model(table_of(pkg, ctx, 15), 64, 2)
    blk = noise(rng, 1, 64)[0]
    assert_same(one(ctx, other, blk, entries), m.process(blk, entries), "a new source after the destroy")
    ctx.destroy_source(other)


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    ctx = pkg.Context(num_bands=3)
    frame, taps, n = 64, 15, 40
    srcs = [ctx.create_source() for _ in range(n)]
    for s in srcs:
        ctx.reflection_render_init(s, frame, taps, 4, 0.01)
    rng = np.random.default_rng(40)
    blk = noise(rng, n, frame)
    lists = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), (1.0, 1.0)) for k in range(3)]] * n
    ctx.reflection_render_process_batch(srcs, blk, lists, stride=4, want_mix=True)
    free0 = device_free_bytes()
    for _ in range(20):
        ctx.reflection_render_process_batch(srcs, blk, lists, stride=4, want_mix=True)
    ctx.reflection_render_process_batch(srcs[:7], blk[:7], lists[:7], stride=3)   # a smaller shape fits what is there
    assert device_free_bytes() >= free0
    ctx.close()


@pytest.mark.gpu
def test_staging_is_its_own(pkg):
    """one "audio callback" = a reverb batch of 2, a direct batch of 5 and a reflection batch of 3, three rounds; each equals what
    it gives alone"""
    frame, taps = 1024, 15
    rng = np.random.default_rng(77)
    irs = [noise_ir(rng, 48000) for _ in range(2)]
    rev_blocks = [noise(rng, 2, frame) * F32(0.3) for _ in range(3)]
    dir_blocks = [noise(rng, 5, frame) for _ in range(3)]
    ref_blocks = [noise(rng, 3, frame) for _ in range(3)]
    tg = [[(float(F32(rng.uniform(0, 400) / FS)), rng.uniform(0, 1, 8).astype(np.float32)) for _ in range(5)] for _ in range(3)]
    lists = [[[entry(k, rng.uniform(0, 400), rng.uniform(0, 1, 8), rng.uniform(-1, 1, 2)) for k in range(2 + cb)] for _ in range(3)]
             for cb in range(3)]

    def run(reverb, direct, reflect):
        ctx = pkg.Context(num_bands=1)
        rs = [ctx.create_source() for _ in range(2)]
        ds = [ctx.create_source() for _ in range(5)]
        es = [ctx.create_source() for _ in range(3)]
        for s, ir in zip(rs, irs):
            ctx.reverb_init(s, frame)
            ctx.set_impulse_response(s, ir)
        for s in ds:
            ctx.direct_render_init(s, frame, taps, 0.01)
        for s in es:
            ctx.reflection_render_init(s, frame, taps, 4, 0.01)
        outs = {"reverb": [], "direct": [], "reflect": []}
        for cb in range(3):
            if reverb:
                outs["reverb"].append(ctx.reverb_process_batch(rs, rev_blocks[cb]).tobytes())
            if direct:
                outs["direct"].append(ctx.direct_render_process_batch(ds, dir_blocks[cb], tg[cb]).tobytes())
            if reflect:
                out, rows = ctx.reflection_render_process_batch(es, ref_blocks[cb], lists[cb])
                outs["reflect"].append(out.tobytes() + rows.tobytes())
        ctx.close()
        return outs

    together = run(True, True, True)
    assert together["reverb"] == run(True, False, False)["reverb"], "the reverb rows changed beside the other batches"
    assert together["direct"] == run(False, True, False)["direct"], "the direct rows changed beside the other batches"
    assert together["reflect"] == run(False, False, True)["reflect"], "the reflection rows changed beside the other batches"


@pytest.mark.gpu
def test_hand_over_between_triangles(pkg):
    """a reflection point that crosses from one triangle of a wall to its neighbour: the key alternates every callback, the delay and
    the gains stay.  Both slots compute the same y, and the linear fade out of one and into the other adds four roundings of
    magnitude <= |y|: within 4 * 2^-24 |y| of the steady voice on a second source, sample by sample"""
    ctx = ctx_for(pkg, 3)
    frame, taps = 320, 15
    a, b = ctx.create_source(), ctx.create_source()
    ctx.reflection_render_init(a, frame, taps, 2, 0.02)
    ctx.reflection_render_init(b, frame, taps, 2, 0.02)
    rng = np.random.default_rng(17)
    gains = rng.uniform(0, 1, 8).astype(np.float32)
    worst = 0.0
    for cb in range(6):
        blk = noise(rng, 1, frame)[0]
        out, rows = ctx.reflection_render_process_batch([a, b], np.stack([blk, blk]), [[entry(1 + cb % 2, 200.4, gains, (1.0, 1.0))],
                                                                                       [entry(9, 200.4, gains, (1.0, 1.0))]])
        if cb == 0:
            assert out[0].tobytes() == out[1].tobytes()
            continue
        assert tuple(int(x) for x in rows[0]) == (2, 1, 1, 0) and tuple(int(x) for x in rows[1]) == (1, 0, 0, 0)
        y = np.abs(out[1].astype(np.float64))   # the steady voice with gains (1, 1) IS y
        diff = np.abs(out[0].astype(np.float64) - out[1].astype(np.float64))
        worst = max(worst, float((diff / np.maximum(4 * EPS * y, 1e-300)).max()))
        assert np.all(diff <= 4 * EPS * y), f"callback {cb + 1}"
    print(f"hand-over: worst share of the bound {worst:.3f}")
    ctx.destroy_source(a)
    ctx.destroy_source(b)


POW2_FS = 65536   # delays of k / 65536 s are exact, and the default edges of eight bands fit under its Nyquist


@pytest.mark.gpu
def test_known_answer(pkg):
    """eight bands with unit gains: the taps are a delta (within the documented 1.3e-8) at c = (T - 1) / 2.  Two held voices at 10
    and 37.5 samples with channel gains (1, 0) and (0, 0.5), an impulse at sample 0: left 1 at c + 10, right 0.25 at c + 37 and
    c + 38, everything else within 4 * 8 * 2^-24"""
    ctx = ctx_for(pkg, 8, POW2_FS)
    frame, taps = 64, 15
    c = (taps - 1) // 2
    src = ctx.create_source()
    ctx.reflection_render_init(src, frame, taps, 2, 0.001)
    ones = np.ones(8, np.float32)
    entries = [(1, 10.0 / POW2_FS, ones, (1.0, 0.0)), (2, 37.5 / POW2_FS, ones, (0.0, 0.5))]
    one(ctx, src, np.zeros(2 * frame, np.float32), entries)   # the voices fade in on silence: held from here on
    blk = np.zeros(2 * frame, np.float32)
    blk[0] = blk[1] = 1.0
    out, row = one(ctx, src, blk, entries)
    assert row == (2, 0, 0, 0)
    want = np.zeros(2 * frame, np.float32)
    want[2 * (c + 10)] = 1.0
    want[2 * (c + 37) + 1] = want[2 * (c + 38) + 1] = 0.25
    assert np.abs(out - want).max() <= 4 * 8 * EPS
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_component_layer(pkg):
    """UpdateReflectionPaths -> FrequenSeeAudioReflectionPlugin.ProcessAudio in the 12-triangle shoebox, the source moved between the
    callbacks: six voices, none dropped, and the C call with Voices()' entries gives the same"""
    w = shoebox_world()
    frame, taps = 64, 15

    def world():
        sub = pkg.AudioRayTracingSubsystem(num_bands=4)
        sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
        sub.SetMaterials(w.absorption, w.transmission, w.scattering)
        comp = pkg.FrequenSeeAudioComponent(SRC)
        comp.OnRegister(sub)
        sub.SetListenerLocation(LIS)
        return sub, comp

    sub, comp = world()
    plug = pkg.FrequenSeeAudioReflectionPlugin(sub)
    plug.Initialize(frame, taps, 16, 0.05)
    plug.OnInitSource(comp)
    sub2, comp2 = world()
    sub2.ctx.reflection_render_init(comp2._src, frame, taps, 16, 0.05)
    rng = np.random.default_rng(2)
    right = [0.0, 1.0, 0.0]
    for cb, pos in enumerate((SRC, [330.0, 240.0, 160.0], [360.0, 250.0, 150.0])):
        comp.SetComponentLocation(pos)
        rows, paths = sub.UpdateReflectionPaths(max_paths=8)
        assert int(rows[0]["returned"]) == 6
        blk = noise(rng, 1, frame)
        got, grow = plug.ProcessAudio([comp], blk, rows, paths, right=right, reference_length=500.0)
        voices = plug.Voices(rows[0], paths[0], right=right, reference_length=500.0)
        assert voices.shape == (6,) and np.array_equal(voices["key"], paths[0]["triangle"][:6])
        want, wrow = sub2.ctx.reflection_render_process_batch([comp2._src], blk, [voices])
        assert int(grow[0]["sounding"]) >= 6 and int(grow[0]["dropped"]) == 0
        if cb == 0:
            assert tuple(int(x) for x in grow[0]) == (6, 6, 0, 0)
        assert got.tobytes() == want.tobytes() and grow.tobytes() == wrow.tobytes()
    assert got.any(), "the shortest reflection (84 samples) is heard by the third block"
    plug.OnReleaseSource(comp)
    sub.Deinitialize()
    sub2.Deinitialize()
