"""fs_direct_render_process_batch: the direct sound of every source of an audio callback — a time-varying fractional delay (the
Doppler shift) and a linear-phase FIR whose taps are sum_b gain_b * k_b (include/frequensee.h, "direct sound on the audio thread").

The yardstick is Model below: a numpy float32 restatement of the header's rule, vectorised over the output sample with a Python
loop over the taps, every operation rounded on its own.  It reads the band table from fs_direct_band_kernels — the very table
fs_direct_render_init uploads — so the device output must EQUAL it (tobytes()).  Beside it: known answers that need no
restatement, the same rule with the multiply-accumulate in float64 under a forward error bound, the batch and state rules, and
the Doppler shift of a sine.
"""
import ctypes as C

import numpy as np
import pytest

from test_direct_paths import LIS, SRC, device_free_bytes, partition_world
from test_reverb_batch import noise_ir

F32 = np.float32
FS = 48000
EPS = 2.0 ** -24


# ---- the band kernels: the header's formula in numpy double -----------------------------------------------------------------
def default_edges(bands):
    return [125.0 * 2.0 ** (b - 0.5) for b in range(1, bands)]


def kernels64(fs, bands, taps, edges=None):
    e = default_edges(bands) if edges is None else [float(F32(x)) for x in edges]
    c = (taps - 1) // 2
    m = np.arange(taps, dtype=np.float64) - c
    w = 0.5 + 0.5 * np.cos(np.pi * m / (c + 1))

    def lowpass(edge):
        if edge == 0:
            return np.zeros(taps)
        if edge == bands:
            return (m == 0).astype(np.float64)
        f = e[edge - 1]
        safe = np.where(m == 0, 1.0, m)
        return np.where(m == 0, 2.0 * f / fs, np.sin(2.0 * np.pi * f * m / fs) / (np.pi * safe))

    return np.stack([w * (lowpass(b + 1) - lowpass(b)) for b in range(bands)])


def delta(taps):
    d = np.zeros(taps, np.float32)
    d[(taps - 1) // 2] = 1.0
    return d


CUSTOM_EDGES = [300.0, 1000.0, 3500.0]


@pytest.mark.parametrize("bands,taps,edges", [(1, 1, None), (3, 15, None), (8, 255, None), (8, 1023, None), (4, 127, CUSTOM_EDGES)])
def test_band_kernels_against_the_formula(pkg, bands, taps, edges):
    k = pkg.Context.direct_band_kernels(FS, bands, taps, edges)
    assert k.shape == (bands, taps) and k.dtype == np.float32
    ref = kernels64(FS, bands, taps, edges)
    ulp = np.maximum(np.spacing(np.abs(ref.astype(np.float32))), np.spacing(np.abs(k))).astype(np.float64)
    assert np.all(np.abs(k.astype(np.float64) - ref) <= ulp), "more than 1 float32 ulp from the formula"
    if bands == 1:
        assert np.array_equal(k[0], delta(taps)), "one band is exactly a delta"
    # linear phase: every kernel is symmetric about its centre, within the rounding of its two halves
    assert np.all(np.abs(k - k[:, ::-1]) <= 2 * np.spacing(np.abs(k)))


def taps32(k, gains):
    """c[t] = sum over b ascending of (c = c + g[b] * k_b[t]), fp32"""
    c = np.zeros(k.shape[1], np.float32)
    for b in range(k.shape[0]):
        c = c + F32(gains[b]) * k[b]
    return c


@pytest.mark.parametrize("bands,taps", [(1, 1), (3, 15), (8, 255), (8, 1023), (8, 2047)])
def test_unit_gains_are_a_delta(pkg, bands, taps):
    k = pkg.Context.direct_band_kernels(FS, bands, taps)
    err = np.abs(taps32(k, np.ones(bands)).astype(np.float64) - delta(taps)).max()
    print(f"bands {bands} taps {taps}: unit-gain taps within {err:.3e} of the delta")
    assert err <= 4 * bands * EPS   # B roundings of values <= 1 plus the table's own


def test_band_kernel_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    buf = np.full((8, 2049), 5.0, np.float32)
    out = buf.ctypes.data

    def call(fs=FS, edges=None, bands=3, taps=15, dest=out):
        e = None if edges is None else np.asarray(edges, np.float32)
        return lib.fs_direct_band_kernels(fs, e.ctypes.data if e is not None else None, bands, taps, dest)

    assert call() == cap.OK
    buf[:] = 5.0
    inf, nan = float("inf"), float("nan")
    assert call(dest=None) == cap.ERR_INVALID_ARGUMENT
    for bands in (0, -1, 9):
        assert call(bands=bands) == cap.ERR_INVALID_ARGUMENT
    for taps in (0, -1, 2, 254, 2048, 2049):
        assert call(taps=taps) == cap.ERR_INVALID_ARGUMENT
    for fs in (0, -48000):
        assert call(fs=fs) == cap.ERR_INVALID_ARGUMENT
    for edges in ([nan, 1000.0], [100.0, inf], [1000.0, 1000.0], [2000.0, 1000.0], [0.0, 1000.0], [-5.0, 1000.0], [1000.0, 24000.0],
                  [1000.0, 30000.0]):
        assert call(edges=edges) == cap.ERR_INVALID_ARGUMENT, edges
    assert call(fs=8000, bands=8) == cap.ERR_INVALID_ARGUMENT, "the default edges of 8 bands do not fit under 4 kHz"
    assert np.all(buf == 5.0), "a refused call wrote"
    assert call(edges=[1000.0, 23999.0]) == cap.OK
    assert call(taps=2047) == cap.OK and call(taps=1, bands=8) == cap.OK
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.direct_band_kernels(FS, 3, 16)


def test_struct_and_exports(pkg):
    cap = pkg._capi
    assert C.sizeof(cap.DirectRenderTarget) == 36 and pkg.Context.RENDER_TARGET_DTYPE.itemsize == 36
    assert cap.DirectRenderTarget.delay.offset == 0 and cap.DirectRenderTarget.band_gain.offset == 4
    assert pkg.Context.RENDER_TARGET_DTYPE.fields["band_gain"][1] == 4
    assert (cap.MAX_DIRECT_RENDER_BATCH, cap.DIRECT_RENDER_MAX_TAPS) == (256, 2047)
    for name in ("fs_direct_band_kernels", "fs_direct_render_init", "fs_direct_render_release", "fs_direct_render_process_batch"):
        assert name in cap.EXPORTS and hasattr(cap.load(), name)
    assert cap.load().fs_abi_version() == 5


def test_null_context_and_null_pointers(pkg):
    cap = pkg._capi
    lib = cap.load()
    src = (C.c_int32 * 1)(0)
    blk = np.zeros(128, np.float32)
    out = np.full(128, 7.0, np.float32)
    tgt = np.zeros(1, dtype=pkg.Context.RENDER_TARGET_DTYPE)
    a, o, t = blk.ctypes.data, out.ctypes.data, tgt.ctypes.data
    assert lib.fs_direct_render_init(None, 0, 64, 15, 0.01) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_direct_render_release(None, 0) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_direct_render_process_batch(None, src, 1, a, t, o, None) == cap.ERR_INVALID_ARGUMENT
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        cfg = cap.default_config(num_bands=1)
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == cap.ERR_NO_DEVICE and h
        try:
            assert lib.fs_direct_render_init(h, 0, 64, 15, 0.01) == cap.ERR_NO_DEVICE
            assert b"no CPU fallback" in lib.fs_last_error(h)
            assert lib.fs_direct_render_process_batch(h, src, 1, a, t, o, None) == cap.ERR_NO_DEVICE
            assert lib.fs_direct_render_process_batch(h, None, 1, a, t, o, None) == cap.ERR_INVALID_ARGUMENT
            assert lib.fs_direct_render_process_batch(h, src, 1, None, t, o, None) == cap.ERR_INVALID_ARGUMENT
            assert lib.fs_direct_render_process_batch(h, src, 1, a, None, o, None) == cap.ERR_INVALID_ARGUMENT
            assert lib.fs_direct_render_process_batch(h, src, 1, a, t, None, None) == cap.ERR_INVALID_ARGUMENT
        finally:
            lib.fs_context_destroy(h)
    assert np.all(out == 7.0)


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
class Model:
    """One source's callback, as include/frequensee.h states it.  process() returns the fp32 output [F * 2]; with want64 also the
    same rule with d, i, f, a from the fp32 rule and every multiply-accumulate in float64, and the bound's sum|c|."""

    def __init__(self, table, frame, fs=FS):
        self.k = np.asarray(table, np.float32)
        self.B, self.T = self.k.shape
        self.F, self.fs = frame, fs
        self.release()

    def release(self):
        self.x = [np.zeros(0, np.float32), np.zeros(0, np.float32)]   # x(n) for n >= 0; zero before
        self.n0 = 0
        self.primed = False

    def sample(self, ch, p):
        """x(p) for an index array p (zero before the stream began)"""
        x = self.x[ch]
        return np.where(p >= 0, x[np.maximum(p, 0)], F32(0.0)).astype(np.float32)

    def process(self, block, delay, gains, want64=False):
        F, T = self.F, self.T
        block = np.asarray(block, np.float32)
        g1 = np.asarray(gains, np.float32)[:self.B]
        d1 = F32(delay) * F32(self.fs)
        if not self.primed:
            self.d0, self.g0 = d1, g1.copy()
        half = F32(0.5) * F32(F)
        e = np.clip(d1 - self.d0, -half, half).astype(np.float32)
        c0, c1 = taps32(self.k, self.g0), taps32(self.k, g1)
        dc = c1 - c0
        s = np.arange(F)
        a = (s + 1).astype(np.float32) / F32(F)
        d = self.d0 + a * e
        fl = np.floor(d)
        f = d - fl
        i = fl.astype(np.int64)
        assert a.dtype == d.dtype == f.dtype == dc.dtype == np.float32
        y = np.zeros(2 * F, np.float32)
        y64 = np.zeros(2 * F, np.float64)
        for ch in range(2):
            self.x[ch] = np.concatenate([self.x[ch], block[ch::2]])
            acc = [np.zeros(F, np.float32) for _ in range(4)]
            acc64 = np.zeros(F, np.float64)
            for t in range(T):
                c = c0[t] + a * dc[t]
                p = self.n0 + s - t - i
                xp, xm = self.sample(ch, p), self.sample(ch, p - 1)
                v = xp + f * (xm - xp)
                acc[t % 4] = acc[t % 4] + c * v
                if want64:
                    c64 = np.float64(c0[t]) + a.astype(np.float64) * (np.float64(c1[t]) - np.float64(c0[t]))
                    acc64 += c64 * (xp.astype(np.float64) + f.astype(np.float64) * (xm.astype(np.float64) - xp.astype(np.float64)))
            y[ch::2] = (acc[0] + acc[1]) + (acc[2] + acc[3])
            y64[ch::2] = acc64
        assert y.dtype == np.float32
        self.n0 += F
        self.d0, self.g0, self.primed = F32(self.d0 + e), g1.copy(), True
        if want64:
            csum = max(np.abs(c0.astype(np.float64)).sum(), np.abs(c1.astype(np.float64)).sum())
            return y, y64, csum
        return y


def noise(rng, count, frame):
    """[count][2 * frame] interleaved stereo, uniform in [-1, 1]: no denormals arise"""
    return rng.uniform(-1.0, 1.0, (count, 2 * frame)).astype(np.float32)


def schedule(frame, bands, rng):
    """six callbacks: primed without a ramp, unchanged, fractional delay up, down with new gains, a jump larger than F/2
    (slew-limited, continuing in the next callback), delay 0 — (delay in seconds, gains)"""
    g_a = rng.uniform(0.0, 1.0, 8).astype(np.float32)
    g_b = rng.uniform(0.0, 1.0, 8).astype(np.float32)
    d = [100.25, 100.25, 110.6, 95.3, 95.3 + 1.7 * frame, 0.0]
    g = [g_a, g_a, g_a, g_b, g_b, g_b]
    return [(float(F32(x / FS)), gg) for x, gg in zip(d, g)]


def test_restatement_against_float64(pkg):
    """the fp32 rule stays inside the forward error bound of T rounded products and sums plus the lerp and tap interpolation:
    |y - y64| <= (T + 8) 2^-24 max|x| max(sum|c0|, sum|c1|), over 60 random cases"""
    rng = np.random.default_rng(0xD1A)
    worst = 0.0
    for case in range(60):
        bands, taps, frame = int(rng.choice([1, 3, 8])), int(rng.choice([15, 63, 255])), 32
        m = Model(pkg.Context.direct_band_kernels(FS, bands, taps), frame)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            y, y64, csum = m.process(blk, float(rng.uniform(0.0, 300.0)) / FS, rng.uniform(0.0, 1.0, 8), want64=True)
        bound = (taps + 8) * EPS * 1.0 * csum
        worst = max(worst, float(np.abs(y - y64).max() / bound))
    print(f"restatement vs float64: worst share of the bound {worst:.3f}")
    assert worst <= 1.0


# ---- GPU -------------------------------------------------------------------------------------------------------------------
_contexts = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _contexts.values():
        ctx.close()
    _contexts.clear()


def ctx_for(pkg, bands, fs=FS):
    """one context per band count and sample rate for the whole module (a source is re-initialised per shape)"""
    key = (bands, fs)
    if key not in _contexts:
        _contexts[key] = pkg.Context(num_bands=bands, sample_rate=fs)
    return _contexts[key]


def table_of(pkg, ctx, taps):
    return pkg.Context.direct_band_kernels(ctx.cfg.sample_rate, ctx.num_bands, taps)


def one(ctx, src, block, delay, gains):
    return ctx.direct_render_process_batch([src], block[None], [(delay, gains)])[0]


# F = 64: a partial tile; 256: exactly one tile; 320: a full tile and a partial one.  T = 5, 9: one tail step behind one and two full
# groups of four (T = 1 never enters the four-wide loop, the other lengths are 3 mod 4)
SHAPES = [(64, 1), (64, 15), (64, 255), (320, 1), (320, 15), (320, 255), (64, 5), (320, 9), (256, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("bands", [1, 3, 8])
@pytest.mark.parametrize("frame,taps", SHAPES)
def test_bit_equal_to_the_restatement(pkg, bands, frame, taps):
    ctx = ctx_for(pkg, bands)
    src = ctx.create_source()
    ctx.direct_render_init(src, frame, taps, 0.02)
    m = Model(table_of(pkg, ctx, taps), frame)
    rng = np.random.default_rng(1000 * bands + frame + taps)
    for cb, (delay, gains) in enumerate(schedule(frame, bands, rng)):
        blk = noise(rng, 1, frame)[0]
        got, want = one(ctx, src, blk, delay, gains), m.process(blk, delay, gains)
        bad = np.nonzero(got != want)[0]
        assert got.tobytes() == want.tobytes(), f"callback {cb + 1}: {bad.size} samples differ, first at {bad[:4]}: {got[bad[:4]]} != {want[bad[:4]]}"
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_longest_filter(pkg):
    ctx = ctx_for(pkg, 8)
    src = ctx.create_source()
    frame, taps = 64, 2047
    ctx.direct_render_init(src, frame, taps, 0.02)
    m = Model(table_of(pkg, ctx, taps), frame)
    rng = np.random.default_rng(2047)
    for cb, (delay, gains) in enumerate(schedule(frame, 8, rng)):
        blk = noise(rng, 1, frame)[0]
        assert one(ctx, src, blk, delay, gains).tobytes() == m.process(blk, delay, gains).tobytes(), f"callback {cb + 1}"
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_ring_wrap(pkg):
    """max delay 400 samples, T = 255, F = 320: the ring is 1024 floats, and eight callbacks write 2560"""
    ctx = ctx_for(pkg, 3)
    src = ctx.create_source()
    frame, taps = 320, 255
    ctx.direct_render_init(src, frame, taps, 400.0 / FS)
    m = Model(table_of(pkg, ctx, taps), frame)
    rng = np.random.default_rng(1024)
    delays = [399.5, 399.5, 250.25, 380.0, 12.5, 399.0, 0.0, 399.75]
    for cb, dl in enumerate(delays):
        blk, gains, delay = noise(rng, 1, frame)[0], rng.uniform(0, 1, 8).astype(np.float32), float(F32(dl / FS))
        assert one(ctx, src, blk, delay, gains).tobytes() == m.process(blk, delay, gains).tobytes(), f"callback {cb + 1}"
    ctx.destroy_source(src)


POW2_FS = 32768   # delays of k / 32768 s are exact: d1 is the whole or half number meant


@pytest.mark.gpu
def test_known_answers(pkg):
    """B = 1, T = 1: the filter is the gain.  Integer delay 37: the input shifted by 37; 37.5: the mean of two neighbours as the
    rule forms it; gain 0: exactly 0"""
    ctx = ctx_for(pkg, 1, POW2_FS)
    frame = 320
    rng = np.random.default_rng(37)
    blocks = noise(rng, 3, frame)
    hist = [np.concatenate([np.zeros(64, np.float32), blocks[:, ch::2].reshape(-1)]) for ch in range(2)]   # x(n) at hist[n + 64]
    for dl, gain in ((37.0, 1.0), (37.5, 1.0), (37.5, 0.0)):
        src = ctx.create_source()
        ctx.direct_render_init(src, frame, 1, 0.01)
        for cb in range(3):
            got = one(ctx, src, blocks[cb], dl / POW2_FS, [gain])
            for ch in range(2):
                p = 64 + cb * frame + np.arange(frame) - int(dl)
                xp, xm = hist[ch][p], hist[ch][p - 1]
                if gain == 0.0:
                    want = np.zeros(frame, np.float32)
                elif dl == 37.0:
                    want = xp
                else:
                    want = xp + F32(0.5) * (xm - xp)
                assert np.array_equal(got[ch::2], want), (dl, gain, cb, ch)
        ctx.destroy_source(src)


@pytest.mark.gpu
def test_against_float64(pkg):
    ctx = ctx_for(pkg, 8)
    src = ctx.create_source()
    frame, taps = 320, 255
    ctx.direct_render_init(src, frame, taps, 0.02)
    m = Model(table_of(pkg, ctx, taps), frame)
    rng = np.random.default_rng(64)
    worst = 0.0
    for cb, (delay, gains) in enumerate(schedule(frame, 8, rng)):
        blk = noise(rng, 1, frame)[0]
        got = one(ctx, src, blk, delay, gains)
        _, y64, csum = m.process(blk, delay, gains, want64=True)
        bound = (taps + 8) * EPS * float(np.abs(blk).max()) * csum
        worst = max(worst, float(np.abs(got - y64).max() / bound))
        assert np.abs(got - y64).max() <= bound, f"callback {cb + 1}"
    print(f"device vs float64: worst share of the bound {worst:.3f}")
    ctx.destroy_source(src)


def mix_model(rows):
    acc = np.asarray(rows[0], np.float32).copy()
    for r in rows[1:]:
        acc = acc + np.asarray(r, np.float32)
    return acc


@pytest.mark.gpu
def test_batch_single_and_permuted_agree(pkg):
    ctx = ctx_for(pkg, 3)
    frame, taps, n = 320, 15, 3
    sets = [[ctx.create_source() for _ in range(n)] for _ in range(3)]   # one call | three calls | permuted order
    for s in sum(sets, []):
        ctx.direct_render_init(s, frame, taps, 0.02)
    models = [Model(table_of(pkg, ctx, taps), frame) for _ in range(n)]
    rng = np.random.default_rng(3)
    perm = [2, 0, 1]
    for cb in range(4):
        blk = noise(rng, n, frame)
        tg = [(float(F32(rng.uniform(0, 600) / FS)), rng.uniform(0, 1, 8).astype(np.float32)) for _ in range(n)]
        out, mix = ctx.direct_render_process_batch(sets[0], blk, tg, want_mix=True)
        singles = [one(ctx, sets[1][i], blk[i], *tg[i]) for i in range(n)]
        pout, pmix = ctx.direct_render_process_batch([sets[2][i] for i in perm], blk[perm], [tg[i] for i in perm], want_mix=True)
        only_mix = None
        for i in range(n):
            want = models[i].process(blk[i], *tg[i])
            assert out[i].tobytes() == want.tobytes(), (cb, i)
            assert singles[i].tobytes() == want.tobytes(), (cb, i)
            assert pout[perm.index(i)].tobytes() == want.tobytes(), (cb, i)
        assert mix.tobytes() == mix_model(out).tobytes(), "mix is not the fp32 sum in list order"
        assert pmix.tobytes() == mix_model(pout).tobytes()
        if cb == 3:   # with out == NULL only the mix comes back; the state moves on all the same
            blk2 = noise(rng, n, frame)
            only_mix = ctx.direct_render_process_batch(sets[0], blk2, tg, want_out=False, want_mix=True)
            assert only_mix.shape == (2 * frame,)
            assert only_mix.tobytes() == mix_model([models[i].process(blk2[i], *tg[i]) for i in range(n)]).tobytes()
    for s in sum(sets, []):
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    cap = pkg._capi
    lib = cap.load()
    ctx = ctx_for(pkg, 3)
    frame, taps = 64, 15
    srcs = [ctx.create_source() for _ in range(3)]
    for s in srcs:
        ctx.direct_render_init(s, frame, taps, 0.01)   # D = 480
    other_frame, other_taps, uninit, dead = (ctx.create_source() for _ in range(4))
    ctx.direct_render_init(other_frame, 128, taps, 0.01)
    ctx.direct_render_init(other_taps, frame, 31, 0.01)
    ctx.direct_render_init(dead, frame, taps, 0.01)
    ctx.destroy_source(dead)
    models = [Model(table_of(pkg, ctx, taps), frame) for _ in range(3)]
    rng = np.random.default_rng(5)
    gains = np.full(8, 0.5, np.float32)

    def good_call():
        blk = noise(rng, 3, frame)
        tg = [(float(F32(rng.uniform(0, 400) / FS)), gains) for _ in range(3)]
        out = ctx.direct_render_process_batch(srcs, blk, tg)
        for i in range(3):
            assert out[i].tobytes() == models[i].process(blk[i], *tg[i]).tobytes(), i

    good_call()
    blk = noise(rng, 3, frame)
    sentinel = np.full((3, 2 * frame), 7.0, np.float32)
    out = sentinel.copy()
    inf, nan = float("inf"), float("nan")

    def call(sources=srcs, count=3, delays=(0.001, 0.002, 0.003), gain=None, blocks=blk, dest=out, mix=None, targets=True):
        arr = (C.c_int32 * len(sources))(*sources)
        t = np.zeros(len(sources), dtype=pkg.Context.RENDER_TARGET_DTYPE)
        for i in range(min(len(sources), len(delays))):
            t[i]["delay"] = delays[i]
            t[i]["band_gain"] = gains if gain is None or i != 1 else gain
        return lib.fs_direct_render_process_batch(ctx.h, arr, count, blocks.ctypes.data if blocks is not None else None,
                                                  t.ctypes.data if targets else None, dest.ctypes.data if dest is not None else None,
                                                  mix.ctypes.data if mix is not None else None)

    bad_gain = lambda v, b=1: np.array([0.5] * b + [v] + [0.5] * (7 - b), np.float32)   # noqa: E731
    for delays in ((0.001, -0.001, 0.003), (0.001, nan, 0.003), (0.001, inf, 0.003), (0.001, 481.0 / FS, 0.003)):
        assert call(delays=delays) == cap.ERR_INVALID_ARGUMENT, delays
    for v in (-0.5, nan, inf):
        assert call(gain=bad_gain(v)) == cap.ERR_INVALID_ARGUMENT, v
    assert call(sources=[srcs[0], srcs[1], srcs[0]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_frame, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_taps, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], uninit, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], dead, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[srcs[0], 12345, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[-1, srcs[1], srcs[2]]) == cap.ERR_BAD_HANDLE
    for count in (0, -1, 257):
        assert call(count=count) == cap.ERR_INVALID_ARGUMENT
    assert call(blocks=None) == cap.ERR_INVALID_ARGUMENT
    assert call(targets=False) == cap.ERR_INVALID_ARGUMENT
    assert call(dest=None) == cap.ERR_INVALID_ARGUMENT, "out == NULL && mix == NULL"
    assert np.array_equal(out, sentinel), "a refused call wrote rows"
    assert call(gain=bad_gain(nan, b=3)) == cap.OK, "entries beyond num_bands are ignored"
    for i in range(3):   # (that call was a callback like any other)
        assert out[i].tobytes() == models[i].process(blk[i], (0.001, 0.002, 0.003)[i], gains).tobytes(), i
    good_call()   # every refused call left all three sources as they were

    # init refusals; a refused init leaves the source as it was
    for args in ((15, 15, 0.01), (16385, 15, 0.01), (frame, 16, 0.01), (frame, 0, 0.01), (frame, 2049, 0.01), (frame, taps, -0.01),
                 (frame, taps, nan), (frame, taps, inf), (frame, taps, 22.0)):
        assert lib.fs_direct_render_init(ctx.h, srcs[0], args[0], args[1], C.c_float(args[2])) == cap.ERR_INVALID_ARGUMENT, args
    assert lib.fs_direct_render_init(ctx.h, 12345, frame, taps, C.c_float(0.01)) == cap.ERR_BAD_HANDLE
    assert lib.fs_direct_render_release(ctx.h, 12345) == cap.ERR_BAD_HANDLE
    assert lib.fs_direct_render_release(ctx.h, uninit) == cap.OK
    good_call()
    for s in srcs + [other_frame, other_taps, uninit]:
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_release_and_reinit(pkg):
    ctx = ctx_for(pkg, 3)
    src = ctx.create_source()
    rng = np.random.default_rng(8)
    frame, taps = 64, 15
    ctx.direct_render_init(src, frame, taps, 0.02)
    gains = rng.uniform(0, 1, 8).astype(np.float32)
    for delay in (0.001, 0.0015):
        one(ctx, src, noise(rng, 1, frame)[0], delay, gains)
    ctx.direct_render_release(src)   # zero history, and the next target is taken without a ramp
    m = Model(table_of(pkg, ctx, taps), frame)
    for delay in (0.012, 0.0121):
        blk = noise(rng, 1, frame)[0]
        assert one(ctx, src, blk, delay, gains).tobytes() == m.process(blk, delay, gains).tobytes()
    for frame, taps in ((320, 15), (64, 255)):   # another F, another T
        ctx.direct_render_init(src, frame, taps, 0.02)
        m = Model(table_of(pkg, ctx, taps), frame)
        for delay in (0.004, 0.0043):
            blk = noise(rng, 1, frame)[0]
            assert one(ctx, src, blk, delay, gains).tobytes() == m.process(blk, delay, gains).tobytes(), (frame, taps)
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_custom_edges_reach_the_kernel(pkg):
    """fs_direct_render_init takes the edges in force: the table of fs_set_band_edges' floats"""
    ctx = pkg.Context(num_bands=4)
    ctx.set_band_edges(CUSTOM_EDGES)
    src = ctx.create_source()
    frame, taps = 64, 127
    ctx.direct_render_init(src, frame, taps, 0.01)
    m = Model(pkg.Context.direct_band_kernels(FS, 4, taps, CUSTOM_EDGES), frame)
    rng = np.random.default_rng(4)
    for delay in (0.002, 0.0021):
        blk, gains = noise(rng, 1, frame)[0], rng.uniform(0, 1, 8).astype(np.float32)
        assert one(ctx, src, blk, delay, gains).tobytes() == m.process(blk, delay, gains).tobytes()
    ctx.close()


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    ctx = pkg.Context(num_bands=3)
    frame, taps, n = 64, 15, 40
    srcs = [ctx.create_source() for _ in range(n)]
    for s in srcs:
        ctx.direct_render_init(s, frame, taps, 0.01)
    rng = np.random.default_rng(40)
    blk = noise(rng, n, frame)
    tg = [(0.001, np.ones(8, np.float32))] * n
    ctx.direct_render_process_batch(srcs, blk, tg, want_mix=True)
    free0 = device_free_bytes()
    ctx.direct_render_process_batch(srcs, blk, tg, want_mix=True)
    ctx.direct_render_process_batch(srcs[:7], blk[:7], tg[:7])   # a smaller count fits what is there
    assert device_free_bytes() >= free0
    ctx.close()


@pytest.mark.gpu
def test_staging_is_not_the_reverbs(pkg):
    """one reverb batch and one direct batch of different counts alternate for four callbacks; each equals its own solo run"""
    frame, taps = 1024, 15
    rng = np.random.default_rng(77)
    irs = [noise_ir(rng, 48000) for _ in range(2)]
    rev_blocks = [noise(rng, 2, frame) * F32(0.3) for _ in range(4)]
    dir_blocks = [noise(rng, 5, frame) for _ in range(4)]
    tg = [[(float(F32(rng.uniform(0, 400) / FS)), rng.uniform(0, 1, 8).astype(np.float32)) for _ in range(5)] for _ in range(4)]

    def run(reverb, direct):
        ctx = pkg.Context(num_bands=1)
        rs = [ctx.create_source() for _ in range(2)]
        ds = [ctx.create_source() for _ in range(5)]
        for s, ir in zip(rs, irs):
            ctx.reverb_init(s, frame)
            ctx.set_impulse_response(s, ir)
        for s in ds:
            ctx.direct_render_init(s, frame, taps, 0.01)
        outs = []
        for cb in range(4):
            if reverb:
                outs.append(ctx.reverb_process_batch(rs, rev_blocks[cb]).tobytes())
            if direct:
                outs.append(ctx.direct_render_process_batch(ds, dir_blocks[cb], tg[cb]).tobytes())
        ctx.close()
        return outs

    both, rev, drc = run(True, True), run(True, False), run(False, True)
    assert both[0::2] == rev, "the reverb rows changed beside a direct batch"
    assert both[1::2] == drc, "the direct rows changed beside a reverb batch"


@pytest.mark.gpu
def test_staging_grows_on_one_side_only(pkg):
    """shape X = 256 sources at frame 16, then shape Y = 8 other sources at frame 640, then X, then Y, in one context: every call's
    output equals that of the same callbacks run alone in a fresh context.  The staging of a call of `count` rows of frame F is
    (blocks 256-byte aligned; an item is 64 bytes, a plan 48, a row 8 F)
      pinned  items [count] | in [count] rows | out [count] rows | mix, one row
      device  items [count] | in [count] rows | plans [count] | out [count] rows | mix, one row
    X: 16 384 + 32 768 + 32 768 + 128 = 82 048 pinned, 16 384 + 32 768 + 12 288 + 32 768 + 128 = 94 336 device;
    Y: 512 + 40 960 + 40 960 + 5 120 = 87 552 pinned, 512 + 40 960 + 512 + 40 960 + 5 120 = 88 064 device.
    From X to Y the pinned side has to grow while the device side must keep its 94 336 bytes: a pair reallocated to what Y asks
    for, its capacities then taken for X's, would let the next X overrun the device block."""
    taps, gains = 15, np.ones(8, np.float32)
    shapes = {"X": (256, 16), "Y": (8, 640)}
    rng = np.random.default_rng(0x51DE)
    calls = [(name, noise(rng, *shapes[name])) for name in "XYXY"]

    def run(names):
        ctx = pkg.Context(num_bands=1)
        srcs = {}
        for name in names:
            count, frame = shapes[name]
            srcs[name] = [ctx.create_source() for _ in range(count)]
            for s in srcs[name]:
                ctx.direct_render_init(s, frame, taps, 0.01)
        outs = [ctx.direct_render_process_batch(srcs[name], blk, [(0.002, gains)] * len(srcs[name]), want_mix=True)
                for name, blk in calls if name in names]
        ctx.close()
        return [out.tobytes() + mix.tobytes() for out, mix in outs]

    both, x, y = run("XY"), run("X"), run("Y")
    assert both[0::2] == x, "the rows of shape X changed beside calls of shape Y"
    assert both[1::2] == y, "the rows of shape Y changed beside calls of shape X"


@pytest.mark.gpu
def test_doppler(pkg):
    """B = 1, T = 1, a 1 kHz sine, the delay shrinking by F / 8 per callback: the source is heard at 1125 Hz"""
    ctx = ctx_for(pkg, 1)
    src = ctx.create_source()
    frame = 1024
    ctx.direct_render_init(src, frame, 1, 0.03)
    n = np.arange(8 * frame)
    tone = np.sin(2.0 * np.pi * 1000.0 * n / FS).astype(np.float32)
    delay = 1024.0
    out = []
    for cb in range(8):   # the first primes at 1024 samples, seven shrink
        blk = np.repeat(tone[cb * frame:(cb + 1) * frame], 2)
        out.append(one(ctx, src, blk, delay / FS, [1.0])[0::2])
        delay -= frame / 8
    y = np.concatenate(out[1:]).astype(np.float64)
    spec = np.abs(np.fft.rfft(y * np.hanning(y.shape[0])))
    peak_hz = float(np.argmax(spec)) * FS / y.shape[0]
    print(f"doppler: spectral peak at {peak_hz:.2f} Hz")
    assert int(np.argmax(spec)) == round(1125.0 * y.shape[0] / FS)
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_component_layer(pkg):
    """FrequenSeeAudioOcclusionPlugin.ProcessAudio equals the direct C call with targets built by hand from UpdateDirectPaths"""
    w = partition_world()
    frame, taps = 64, 15

    def world():
        sub = pkg.AudioRayTracingSubsystem(num_bands=4)
        sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
        sub.SetMaterials(w.absorption, w.transmission)
        comps = [pkg.FrequenSeeAudioComponent(p) for p in (SRC, [700.0, 100.0, 50.0])]
        for c in comps:
            c.OnRegister(sub)
        sub.SetListenerLocation(LIS)
        return sub, comps

    sub, comps = world()
    plug = pkg.FrequenSeeAudioOcclusionPlugin(sub)
    plug.Initialize(frame, taps, 0.05)
    for c in comps:
        plug.OnInitSource(c)
    paths = sub.UpdateDirectPaths(samples=16, source_radius=30.0)
    assert paths[0]["surfaces"] == 2 and paths[1]["surfaces"] == 0
    sub2, comps2 = world()
    for c in comps2:
        sub2.ctx.direct_render_init(c._src, frame, taps, 0.05)
    tg = np.zeros(2, dtype=pkg.Context.RENDER_TARGET_DTYPE)
    for i in range(2):
        tg[i]["delay"] = max(float(paths[i]["delay"]) - ((taps - 1) // 2) / FS, 0.0)
        tg[i]["band_gain"] = paths[i]["transmission"]
    assert tg[0]["delay"] > 0 and np.array_equal(tg[0]["band_gain"][:4], paths[0]["transmission"][:4])
    rng = np.random.default_rng(2)
    models = [Model(pkg.Context.direct_band_kernels(FS, 4, taps), frame) for _ in range(2)]
    for cb in range(2):
        blk = noise(rng, 2, frame)
        got, mix = plug.ProcessAudio(comps, blk, paths, want_mix=True)
        want = sub2.ctx.direct_render_process_batch([c._src for c in comps2], blk, tg)
        assert got.tobytes() == want.tobytes()
        assert mix.tobytes() == mix_model(want).tobytes()
        for i in range(2):
            assert got[i].tobytes() == models[i].process(blk[i], tg[i]["delay"], tg[i]["band_gain"]).tobytes()
    plug.OnReleaseSource(comps[0])
    sub.Deinitialize()
    sub2.Deinitialize()
