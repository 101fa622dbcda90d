"""fs_binaural_render_process_batch: every discrete path of a source rendered from its arrival direction — the reflection renderer's
voice bank with one gain per voice and, per ear, the head-related impulse response of the set direction nearest to the voice's
direction folded into the voice's band FIR (include/frequensee.h, "binaural voices on the audio thread").

The yardstick is Model below: a numpy float32 restatement of the header's rule — slot matching, the argmax over the set with its
ties, the fold of the HRIR into the band FIR, the tap loop — which the device must EQUAL (tobytes()).  Beside it two yardsticks the
new code did not write (the reflection and the direct renderer on the device, which a set of H = 1 with taps of 1 must reproduce),
the same rule in float64 under a derived bound, known answers that need no restatement, and the batch, state and refusal rules.
"""
import ctypes as C

import numpy as np
import pytest

from test_direct_paths import device_free_bytes
from test_direct_render import EPS, F32, FS
from test_direct_render import _close_contexts  # noqa: F401  (closes the contexts ctx_for caches when this module is done)
from test_direct_render import ctx_for, mix_model, noise, schedule, table_of, taps32
from test_reflection_paths import LIS, SRC, shoebox_world
from test_reflection_render import POW2_FS, bank_schedule, secs
from test_reverb_batch import noise_ir

MAX_VOICES = 32
DIRECT_KEY = 0x1FFFFFFF


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def nearest(dirs, d):
    """rule 2: the lowest index that maximises (d.x p.x + d.y p.y) + d.z p.z, fp32"""
    p = np.asarray(dirs, np.float32)
    d = np.asarray(d, np.float32)
    dot = (d[0] * p[:, 0] + d[1] * p[:, 1]) + d[2] * p[:, 2]
    assert dot.dtype == np.float32
    return int(np.argmax(dot))   # (the first of equal maxima)


def fold32(h, f):
    """rule 3: C[u] = the sum from 0 over k ascending from max(0, u - T + 1) to min(H - 1, u) of acc = acc + h[k] * f[u - k], fp32.
    Vectorised over u with f zero-padded: a product with a padding zero is +-0, and acc + (+-0) has acc's bits because acc, which
    starts at +0, is never -0 (a sum is -0 only when both terms are)."""
    h, f = np.asarray(h, np.float32), np.asarray(f, np.float32)
    H, T = h.shape[0], f.shape[0]
    pad = np.concatenate([np.zeros(H - 1, np.float32), f, np.zeros(H - 1, np.float32)])
    acc = np.zeros(T + H - 1, np.float32)
    u = np.arange(T + H - 1)
    for k in range(H):
        acc = acc + h[k] * pad[u - k + H - 1]
    assert acc.dtype == np.float32
    return acc


def fold_by_the_letter(h, f):
    """rule 3 as written, one scalar at a time"""
    H, T = len(h), len(f)
    out = np.zeros(T + H - 1, np.float32)
    for u in range(T + H - 1):
        acc = F32(0.0)
        for k in range(max(0, u - T + 1), min(H - 1, u) + 1):
            acc = F32(acc + F32(F32(h[k]) * F32(f[u - k])))
        out[u] = acc
    return out


class Model:
    """One source's callback, as include/frequensee.h states it.  An entry is (key, delay in s, band gains, gain, direction).
    process() returns (the fp32 output [F * 2], the row's counts (sounding, started, ended, dropped)); with want64 also the same rule
    with d, i, f, a and the HRIR indices from the fp32 rule and the fold, the coefficients and every multiply-accumulate in
    float64, and the two weights of the bound (test_restatement_against_float64)."""

    def __init__(self, table, dirs, hrir, frame, voices, fs=FS):
        self.k = np.asarray(table, np.float32)
        self.B, self.T = self.k.shape
        self.F, self.V, self.fs = frame, voices, fs
        self.set(dirs, hrir)
        self.release()

    def set(self, dirs, hrir):
        """fs_hrtf_set: every held slot is free, the history stays"""
        self.dirs, self.hrir = np.asarray(dirs, np.float32), np.asarray(hrir, np.float32)
        self.H = self.hrir.shape[2]
        self.slots = [None] * self.V

    def release(self):
        self.x = [np.zeros(0, np.float32), np.zeros(0, np.float32)]   # x(n) for n >= 0; zero before
        self.n0 = 0
        self.slots = [None] * self.V   # None = free, else dict(key, d0, g0, w0, q0)

    def sample(self, ch, p):
        x = self.x[ch]
        return np.where(p >= 0, x[np.maximum(p, 0)], F32(0.0)).astype(np.float32)

    def match(self, entries):
        """rules 1 and 2: per slot None or (kind, d0, g0, w0, q0, d1, g1, w1, q1, key), and the counts"""
        plan = [None] * self.V
        started = ended = dropped = 0
        target = {}
        for key, delay, gains, gain, direction in entries:
            assert key not in target
            target[key] = (F32(delay) * F32(self.fs), np.asarray(gains, np.float32)[:self.B].copy(), F32(gain), nearest(self.dirs, direction))
        free = [j for j in range(self.V) if self.slots[j] is None]   # as the callback began
        for j, st in enumerate(self.slots):
            if st is None:
                continue
            if st["key"] in target:
                d1, g1, w1, q1 = target.pop(st["key"])
                plan[j] = ("continue", st["d0"], st["g0"], st["w0"], st["q0"], d1, g1, w1, q1, st["key"])
            else:
                plan[j] = ("end", st["d0"], st["g0"], st["w0"], st["q0"], st["d0"], st["g0"], F32(0.0), st["q0"], st["key"])
                ended += 1
        for key, (d1, g1, w1, q1) in target.items():   # (a dict keeps the list order)
            if free:
                plan[free.pop(0)] = ("start", d1, g1, F32(0.0), q1, d1, g1, w1, q1, key)
                started += 1
            else:
                dropped += 1
        return plan, (sum(p is not None for p in plan), started, ended, dropped)

    def process(self, block, entries, want64=False):
        F, Tc = self.F, self.T + self.H - 1
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
        weight_loop = weight_fold = 0.0
        k64 = self.k.astype(np.float64)
        for j, p in enumerate(plan):   # ascending slot number
            if p is None:
                continue
            kind, d0, g0, w0, q0, d1, g1, w1, q1, key = p
            e = np.clip(d1 - d0, -half, half).astype(np.float32)
            f0, f1 = taps32(self.k, g0), taps32(self.k, g1)
            d = d0 + a * e
            fl = np.floor(d)
            f = d - fl
            i = fl.astype(np.int64)
            dw = F32(w1 - w0)
            w = w0 + a * dw
            assert a.dtype == d.dtype == f.dtype == w.dtype == np.float32
            loop_sum = fold_sum = 0.0
            for ch in range(2):
                c0, c1 = fold32(self.hrir[q0, ch], f0), fold32(self.hrir[q1, ch], f1)
                dc = c1 - c0
                assert dc.dtype == np.float32 and dc.shape == (Tc,)
                if want64:
                    h0, h1 = self.hrir[q0, ch].astype(np.float64), self.hrir[q1, ch].astype(np.float64)
                    e0, e1 = np.convolve(h0, g0.astype(np.float64) @ k64), np.convolve(h1, g1.astype(np.float64) @ k64)
                    loop_sum = max(loop_sum, np.abs(c0.astype(np.float64)).sum(), np.abs(c1.astype(np.float64)).sum())
                    fold_sum = max(fold_sum, np.abs(h0).sum() * (np.abs(g0.astype(np.float64)) @ np.abs(k64)).sum(),
                                   np.abs(h1).sum() * (np.abs(g1.astype(np.float64)) @ np.abs(k64)).sum())
                acc = [np.zeros(F, np.float32) for _ in range(4)]
                acc64 = np.zeros(F, np.float64)
                for t in range(Tc):
                    c = c0[t] + a * dc[t]
                    q = self.n0 + s - t - i
                    xp, xm = self.sample(ch, q), self.sample(ch, q - 1)
                    v = xp + f * (xm - xp)
                    acc[t % 4] = acc[t % 4] + c * v
                    if want64:
                        c64 = e0[t] + a64 * (e1[t] - e0[t])
                        acc64 += c64 * (xp.astype(np.float64) + f.astype(np.float64) * (xm.astype(np.float64) - xp.astype(np.float64)))
                y = (acc[0] + acc[1]) + (acc[2] + acc[3])
                assert y.dtype == np.float32
                out[ch::2] = out[ch::2] + w * y
                out64[ch::2] += (np.float64(w0) + a64 * (np.float64(w1) - np.float64(w0))) * acc64
            wmax = float(max(abs(w0), abs(w1)))
            weight_loop += wmax * loop_sum
            weight_fold += wmax * fold_sum
            if kind == "end":
                self.slots[j] = None
            else:
                g_after = np.zeros(self.B, np.float32)
                g_after[:] = g1
                self.slots[j] = dict(key=key, d0=F32(d0 + e), g0=g_after, w0=F32(w1), q0=q1)
        assert out.dtype == np.float32
        self.n0 += F
        if want64:
            return out, row, out64, weight_loop, weight_fold
        return out, row


def bound64(T, H, B, K, weight_loop, weight_fold, peak=1.0):
    """|y - y64| <= 2^-24 max|x| ((Tc + 8 + K + 2) W_loop + (H + B + 2) W_fold).
    The first term is the reflection renderer's derived bound with Tc = T + H - 1 taps: per voice Tc rounded products and sums plus
    the coefficient's lerp and the tap interpolation (Tc + 8), one rounding per product and per sum of the K voices' weighted sum and
    the gain ramp's two (K + 2), relative to W_loop = sum_j max(|w0_j|, |w1_j|) max over ears and ends of sum_u |C[u]|.
    The second is the folded table's own rounding against the exact fold: f[t] is a dot product over B bands and C[u] one over at
    most H taps of h on top of it — a relative error of at most (1 + u)^(B + H) - 1 <= (H + B + 1) u (1 + ...) of the sum of the
    products' magnitudes, sum_k |h[k]| sum_b |g_b k_b[u - k]| — and dC = C1 - C0 rounds once more: (H + B + 2) u, relative to
    W_fold = sum_j max(|w0_j|, |w1_j|) max over ears and ends of (sum |h|) (sum_t sum_b |g_b k_b[t]|) >= sum_u of those magnitudes."""
    return EPS * peak * ((T + H - 1 + 8 + K + 2) * weight_loop + (H + B + 2) * weight_fold)


def entry(key, samples, gains, gain, direction, fs=FS):
    return (key, secs(samples, fs), np.asarray(gains, np.float32), float(F32(gain)), np.asarray(direction, np.float32))


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)


def make_set(pkg, n, H, rng, fs=FS):
    """a set of n directions and random HRIRs of H taps: n = 1: +x; n = 6: the axes, from which (1, 1, 0) is as far from +x as
    from +y; n = 258: the spherical head's directions with 200 := 100 (two equal directions: the lower index wins)"""
    if n == 1:
        dirs = AXES[:1].copy()
    elif n == 6:
        dirs = AXES.copy()
    else:
        dirs = pkg.Context.hrtf_spherical_head(fs, n, 64)[0]
        dirs[200] = dirs[100]
    return dirs, rng.uniform(-1.0, 1.0, (n, 2, H)).astype(np.float32)


def ones_set():
    """H = 1, every tap 1.0f: the fold is the identity"""
    return AXES.copy(), np.ones((6, 2, 1), np.float32)


def tie_directions(dirs):
    """queries with two equal maxima, and what they must resolve to"""
    if dirs.shape[0] == 6:
        return [((1.0, 1.0, 0.0), 0), ((-1.0, 0.0, -1.0), 1), ((0.0, 2.0, 2.0), 2)]
    if dirs.shape[0] == 258:
        return [(tuple(dirs[100]), 100), (tuple(dirs[200] * F32(3.0)), 100)]
    return [((0.0, 1.0, 0.0), 0), ((-5.0, 0.0, 0.0), 0)]


def test_nearest_resolves_ties_to_the_lower_index(pkg):
    rng = np.random.default_rng(1)
    for n in (1, 6, 258):
        dirs, _ = make_set(pkg, n, 1, rng)
        for d, want in tie_directions(dirs):
            assert nearest(dirs, d) == want, (n, d)


def test_fold_restatements_agree(pkg):
    """the vectorised fold the yardstick uses has the bits of the rule taken by the letter — on random taps and on the spherical
    head's own (an onset of zeros, then a decaying tail); H = 1 with a tap of 1 is the identity"""
    rng = np.random.default_rng(2)
    head = pkg.Context.hrtf_spherical_head(FS, 6, 40)[1]
    for k, ear in ((0, 0), (2, 0), (2, 1)):
        f = rng.uniform(-1, 1, 15).astype(np.float32)
        assert fold32(head[k, ear], f).tobytes() == fold_by_the_letter(head[k, ear], f).tobytes(), (k, ear)
    for H, T in ((1, 1), (1, 15), (2, 1), (7, 15), (16, 5), (5, 5)):
        h, f = rng.uniform(-1, 1, H).astype(np.float32), rng.uniform(-1, 1, T).astype(np.float32)
        h[rng.integers(0, H)] = 0.0
        assert fold32(h, f).tobytes() == fold_by_the_letter(h, f).tobytes(), (H, T)
    f = rng.uniform(-1, 1, 15).astype(np.float32)
    assert fold32(np.ones(1, np.float32), f).tobytes() == f.tobytes()


def test_restatement_against_float64(pkg):
    """bound64, derived there, not measured.  40 random cases, K <= 3 voices, the second callback ramping delays, gains and
    directions; the worst observed share of the bound is printed (DESIGN.md records it)"""
    rng = np.random.default_rng(0xB1A0)
    worst = 0.0
    for case in range(40):
        bands, taps, H, frame = int(rng.choice([1, 3, 8])), int(rng.choice([15, 63])), int(rng.choice([2, 7, 32])), 32
        K = int(rng.integers(1, 4))
        dirs, hrir = make_set(pkg, 258 if case % 2 else 6, H, rng)
        m = Model(pkg.Context.direct_band_kernels(FS, bands, taps), dirs, hrir, frame, K)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            entries = [(k, float(rng.uniform(0.0, 300.0)) / FS, rng.uniform(0.0, 1.0, 8), float(rng.uniform(-1.0, 1.0)), rng.normal(size=3))
                       for k in range(K)]
            y, row, y64, w_loop, w_fold = m.process(blk, entries, want64=True)
        assert row == (K, 0, 0, 0)
        worst = max(worst, float(np.abs(y - y64).max() / bound64(taps, H, bands, K, w_loop, w_fold)))
    print(f"restatement vs float64: worst share of the bound {worst:.3f}")
    assert worst <= 1.0


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def one(ctx, src, block, entries, **kw):
    out, rows = ctx.binaural_render_process_batch([src], block[None], [entries], **kw)
    return out[0], tuple(int(x) for x in rows[0])


def assert_same(got, want, where):
    (g, grow), (w, wrow) = got, want
    assert grow == wrow, f"{where}: rows {grow} != {wrow}"
    bad = np.nonzero(g != w)[0]
    assert g.tobytes() == w.tobytes(), f"{where}: {bad.size} samples differ, first at {bad[:4]}: {g[bad[:4]]} != {w[bad[:4]]}"


def binaural_schedule(rng, dirs):
    """the reflection renderer's eight-callback script on three slots (bank_schedule: start | steady | ramps, one gain negative | a
    key vanishing while another starts | the key returning in a permuted list | a fourth entry dropped | all ending | silence) with
    the first channel gain as the gain and a direction per entry: steady over the first two callbacks, then a new one in every
    callback — the HRIR crossfades — among them the set's tie queries"""
    ties = [d for d, _ in tie_directions(dirs)]
    fixed = {}
    script = []
    for cb, (entries, counts) in enumerate(bank_schedule(rng)):
        lst = []
        for e, (key, delay, gains, chan) in enumerate(entries):
            if cb < 2:
                d = fixed.setdefault(key, rng.normal(size=3))
            elif (cb + e) % 3 == 0:
                d = ties[(cb + e) % len(ties)]
            else:
                d = rng.normal(size=3)
            lst.append((key, delay, gains, float(chan[0]), np.asarray(d, np.float32)))
        script.append((lst, counts))
    return script


# every B, F, T, H and n the rule names at least once, the large ones (T = 255, H = 128) together and apart, each small value with
# both frame sizes: (bands, frame, taps, H, n).  F = 320: the second tile has 64 of its 256 threads live.
SHAPES = [(1, 64, 1, 1, 1), (3, 64, 15, 2, 6), (8, 64, 255, 7, 258), (8, 320, 15, 128, 258), (3, 320, 255, 128, 6), (1, 320, 1, 7, 6),
          (3, 64, 1, 128, 1), (8, 320, 255, 1, 258), (1, 64, 15, 7, 258), (3, 320, 15, 2, 1), (8, 64, 1, 2, 6), (1, 320, 255, 2, 258)]


@pytest.mark.gpu
@pytest.mark.parametrize("bands,frame,taps,H,n", SHAPES)
def test_bit_equal_to_the_restatement(pkg, bands, frame, taps, H, n):
    ctx = ctx_for(pkg, bands)
    rng = np.random.default_rng(1000 * bands + frame + taps + 7 * H + n)
    dirs, hrir = make_set(pkg, n, H, rng)
    ctx.hrtf_set(dirs, hrir)
    assert ctx.hrtf_info() == (n, H)
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, taps, 3, 0.02)
    m = Model(table_of(pkg, ctx, taps), dirs, hrir, frame, 3)
    for cb, (entries, counts) in enumerate(binaural_schedule(rng, dirs)):
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
def test_ties_on_the_device(pkg):
    """a steady voice at a tie query sounds exactly like one aimed at the lower of the two indices"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(6)
    frame, taps = 64, 15
    for n in (6, 258):
        dirs, hrir = make_set(pkg, n, 7, rng)
        ctx.hrtf_set(dirs, hrir)
        ties = tie_directions(dirs)
        a, b = ctx.create_source(), ctx.create_source()
        for s in (a, b):
            ctx.binaural_render_init(s, frame, taps, len(ties), 0.02)
        g = rng.uniform(0, 1, 8).astype(np.float32)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            at_tie = one(ctx, a, blk, [entry(k, 30.5, g, 0.7, d) for k, (d, _) in enumerate(ties)])
            at_index = one(ctx, b, blk, [entry(k, 30.5, g, 0.7, dirs[q]) for k, (_, q) in enumerate(ties)])
            assert_same(at_tie, at_index, f"n = {n}, callback {cb + 1}")
        assert at_tie[0].any()
        ctx.destroy_source(a)
        ctx.destroy_source(b)


@pytest.mark.gpu
def test_longest_filter(pkg):
    """Tc = FS_DIRECT_RENDER_MAX_TAPS: T = 2047 with H = 1 is accepted and right, T = 2047 with H = 2 is refused, T = 1921 with
    H = 127 is the same Tc from the other side"""
    cap = pkg._capi
    ctx = ctx_for(pkg, 8)
    src = ctx.create_source()
    rng = np.random.default_rng(2047)
    frame = 64
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    dirs2, hrir2 = make_set(pkg, 6, 2, rng)
    ctx.hrtf_set(dirs2, hrir2)
    assert ctx.lib.fs_binaural_render_init(ctx.h, src, frame, 2047, 2, C.c_float(0.02)) == cap.ERR_INVALID_ARGUMENT
    for taps, H in ((2047, 1), (1921, 127)):
        dirs, hrir = make_set(pkg, 6, H, rng)
        ctx.hrtf_set(dirs, hrir)
        ctx.binaural_render_init(src, frame, taps, 2, 0.02)
        m = Model(table_of(pkg, ctx, taps), dirs, hrir, frame, 2)
        for cb, (da, db) in enumerate(((300.5, 10.0), (310.25, 4.75))):
            blk = noise(rng, 1, frame)[0]
            entries = [entry(1, da, g[0], 0.9, rng.normal(size=3)), entry(2, db, g[1], -0.3, rng.normal(size=3))]
            assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"T = {taps}, H = {H}, callback {cb + 1}")
    # the set grows under an initialised source: Tc would be 2048, and the callback is refused until the source is initialised anew
    ctx.hrtf_set(*ones_set())
    ctx.binaural_render_init(src, frame, 2047, 2, 0.02)
    ctx.hrtf_set(dirs2, hrir2)
    with pytest.raises(pkg.FrequenSeeError) as ei:
        one(ctx, src, noise(rng, 1, frame)[0], [entry(1, 10.0, g[0], 1.0, (1.0, 0.0, 0.0))])
    assert ei.value.code == cap.ERR_INVALID_ARGUMENT
    ctx.binaural_render_init(src, frame, 15, 2, 0.02)
    assert one(ctx, src, noise(rng, 1, frame)[0], [entry(1, 10.0, g[0], 1.0, (1.0, 0.0, 0.0))])[1] == (1, 1, 0, 0)
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_ones_set_is_the_reflection_renderer(pkg):
    """the yardstick the new code did not write: with a set of H = 1 whose taps are 1.0f the fold is the identity, and the output
    equals fs_reflection_render_process_batch with channel_gain = (gain, gain), by value, over the eight-callback script"""
    for bands, frame, taps in ((3, 64, 15), (8, 320, 255), (1, 320, 1)):
        ctx = ctx_for(pkg, bands)
        ctx.hrtf_set(*ones_set())
        a, b = ctx.create_source(), ctx.create_source()
        ctx.binaural_render_init(a, frame, taps, 3, 0.02)
        ctx.reflection_render_init(b, frame, taps, 3, 0.02)
        rng = np.random.default_rng(frame + taps)
        heard = False
        for cb, (entries, counts) in enumerate(bank_schedule(rng)):
            blk = noise(rng, 1, frame)[0]
            got = one(ctx, a, blk, [(key, delay, gains, float(chan[0]), rng.normal(size=3)) for key, delay, gains, chan in entries])
            want, wrow = ctx.reflection_render_process_batch([b], blk[None], [[(key, delay, gains, (chan[0], chan[0])) for key, delay, gains, chan in entries]])
            assert got[1] == counts == tuple(int(x) for x in wrow[0])
            assert np.array_equal(got[0], want[0]), f"bands {bands}, F {frame}, T {taps}, callback {cb + 1}"
            heard = heard or bool(got[0].any())
        assert heard
        ctx.destroy_source(a)
        ctx.destroy_source(b)


@pytest.mark.gpu
def test_one_voice_on_the_ones_set_is_the_direct_renderer(pkg):
    """source A: one voice with gain 1 on the H = 1 set of ones; source B: fs_direct_render_process_batch; the same input and
    targets.  From the second callback on (the first fades in) the outputs are equal by value"""
    ctx = ctx_for(pkg, 3)
    ctx.hrtf_set(*ones_set())
    frame, taps = 320, 15
    a, b = ctx.create_source(), ctx.create_source()
    ctx.binaural_render_init(a, frame, taps, 2, 0.02)
    ctx.direct_render_init(b, frame, taps, 0.02)
    rng = np.random.default_rng(8)
    for cb, (delay, gains) in enumerate(schedule(frame, 3, rng)):
        blk = noise(rng, 1, frame)[0]
        got, row = one(ctx, a, blk, [(5, delay, gains, 1.0, rng.normal(size=3))])
        want = ctx.direct_render_process_batch([b], blk[None], [(delay, gains)])[0]
        assert row == (1, 1 if cb == 0 else 0, 0, 0)
        if cb:
            assert np.array_equal(got, want), f"callback {cb + 1}"
            assert got.any()
    ctx.destroy_source(a)
    ctx.destroy_source(b)


@pytest.mark.gpu
def test_full_bank(pkg):
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(32)
    frame, taps = 64, 15
    dirs, hrir = make_set(pkg, 258, 7, rng)
    ctx.hrtf_set(dirs, hrir)
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, taps, MAX_VOICES, 0.02)
    m = Model(table_of(pkg, ctx, taps), dirs, hrir, frame, MAX_VOICES)
    for cb in range(3):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(1000 + k, rng.uniform(0, 900), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(MAX_VOICES)]
        got = one(ctx, src, blk, entries)
        assert got[1] == (32, 32 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_ring_wrap(pkg):
    """max delay 400 samples, Tc = 15 + 7 - 1, F = 320: the ring is 1024 floats, and twenty callbacks write 6400"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(1024)
    frame, taps = 320, 15
    dirs, hrir = make_set(pkg, 6, 7, rng)
    ctx.hrtf_set(dirs, hrir)
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, taps, 3, 400.0 / FS)
    m = Model(table_of(pkg, ctx, taps), dirs, hrir, frame, 3)
    for cb in range(20):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(k, x, rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k, x in ((1, 400.0), (2, rng.uniform(0, 400)))]
        if cb % 5 == 4:
            entries = entries[:1]   # the second voice ends, and starts again in the next callback
        assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


# ---- physics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_interaural_delay_of_delta_hrirs(pkg):
    """HRIRs that are a delta at tap 3 (left) and tap 10 (right), one band (its kernel of T = 1 is exactly 1), unit gains, a held
    voice at 20 samples: an impulse at sample 0 of both channels comes out as exactly 1 at 20 + 3 left and 20 + 10 right — seven
    samples of interaural delay — and exactly 0 elsewhere"""
    ctx = ctx_for(pkg, 1, POW2_FS)
    hrir = np.zeros((1, 2, 11), np.float32)
    hrir[0, 0, 3] = hrir[0, 1, 10] = 1.0
    ctx.hrtf_set(AXES[:1], hrir)
    frame = 64
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, 1, 2, 0.001)
    entries = [(1, 20.0 / POW2_FS, np.ones(8, np.float32), 1.0, (0.3, -0.2, 0.9))]
    one(ctx, src, np.zeros(2 * frame, np.float32), entries)   # the voice fades in on silence: held from here on
    blk = np.zeros(2 * frame, np.float32)
    blk[0] = blk[1] = 1.0
    out, row = one(ctx, src, blk, entries)
    assert row == (1, 0, 0, 0)
    want = np.zeros(2 * frame, np.float32)
    want[2 * (20 + 3)] = want[2 * (20 + 10) + 1] = 1.0
    assert np.array_equal(out, want)
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_alternating_direction_is_a_crossfade(pkg):
    """source A's one voice points at +y and -y in turn; B and C hold it steadily at +y and at -y; the same input, delay and
    gains.  The coefficient C0[u] + a dC[u] is linear in the two tables, so in exact arithmetic A = (1 - a) y_q0 + a y_q1 sample by
    sample.  The comparison is held to bound64 (K = 1) itself, the float64 bound of one voice with these gains and tables, sample by
    sample; the block's last sample has a = 1 and is within that bound of the steady q1 voice's.  No voice starts or ends."""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(17)
    frame, taps, H = 320, 15, 7
    dirs, hrir = make_set(pkg, 6, H, rng)   # +y is index 2, -y index 3
    ctx.hrtf_set(dirs, hrir)
    srcs = [ctx.create_source() for _ in range(3)]
    for s in srcs:
        ctx.binaural_render_init(s, frame, taps, 2, 0.02)
    gains = rng.uniform(0, 1, 8).astype(np.float32)
    k = table_of(pkg, ctx, taps)
    f = taps32(k, gains)
    loop = max(np.abs(fold32(hrir[q, ear], f).astype(np.float64)).sum() for q in (2, 3) for ear in (0, 1))
    fold = max(np.abs(hrir[q, ear].astype(np.float64)).sum() for q in (2, 3) for ear in (0, 1)) * \
        (np.abs(gains[:3].astype(np.float64)) @ np.abs(k.astype(np.float64))).sum()
    bound = bound64(taps, H, 3, 1, loop, fold)
    a = np.repeat(((np.arange(frame) + 1).astype(np.float32) / F32(frame)).astype(np.float64), 2)
    y_dir = [(0.0, 1.0, 0.0), (0.0, -1.0, 0.0)]
    worst = 0.0
    for cb in range(6):
        blk = noise(rng, 1, frame)[0]
        q0, q1 = (cb + 1) % 2, cb % 2   # what A comes from and goes to
        out, rows = ctx.binaural_render_process_batch(srcs, np.stack([blk] * 3), [[entry(1, 200.4, gains, 1.0, y_dir[q1])],
                                                                                  [entry(1, 200.4, gains, 1.0, y_dir[0])],
                                                                                  [entry(1, 200.4, gains, 1.0, y_dir[1])]])
        if cb == 0:
            continue   # all three fade in
        assert [tuple(int(x) for x in r) for r in rows] == [(1, 0, 0, 0)] * 3
        steady = [out[1].astype(np.float64), out[2].astype(np.float64)]
        diff = np.abs(out[0].astype(np.float64) - ((1.0 - a) * steady[q0] + a * steady[q1]))
        worst = max(worst, float(diff.max() / bound))
        assert np.all(diff <= bound), f"callback {cb + 1}"
        assert np.all(np.abs(out[0][-2:].astype(np.float64) - steady[q1][-2:]) <= bound), "the block's last sample is the new direction's"
        assert np.abs(steady[0] - steady[1]).max() > 100 * bound, "the two directions sound different"
    print(f"alternating direction: worst share of the bound {worst:.3f}")
    for s in srcs:
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_spherical_head_puts_the_sound_on_its_side(pkg):
    """fs_hrtf_spherical_head (n = 258, H = 64), a 1 kHz sine in both channels, four callbacks: a voice from +y is louder in the
    right ear, one from -y in the left.  By value: on the set mirrored in y (every direction's y negated, its ears swapped) the
    voice from -y gives the first voice's output with the channels swapped"""
    ctx = ctx_for(pkg, 3)
    frame, taps = 320, 15
    dirs, hrir = pkg.Context.hrtf_spherical_head(FS, 258, 64)
    mirrored = (dirs * np.array([1.0, -1.0, 1.0], np.float32), np.ascontiguousarray(hrir[:, ::-1, :]))
    t = np.arange(4 * frame) / FS
    sine = np.repeat(np.sin(2 * np.pi * 1000.0 * t).astype(np.float32), 2).reshape(4, 2 * frame)
    ones = np.ones(8, np.float32)

    def run(the_set, direction):
        ctx.hrtf_set(*the_set)
        src = ctx.create_source()
        ctx.binaural_render_init(src, frame, taps, 2, 0.02)
        outs = [one(ctx, src, sine[cb], [entry(1, 40.0, ones, 1.0, direction)])[0] for cb in range(4)]
        ctx.destroy_source(src)
        return np.stack(outs)

    def rms(x):
        return float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))

    from_right = run((dirs, hrir), (0.0, 1.0, 0.0))
    from_left = run((dirs, hrir), (0.0, -1.0, 0.0))
    last = from_right[3]
    print(f"from +y: rms left {rms(last[0::2]):.4f} right {rms(last[1::2]):.4f}; from -y: left {rms(from_left[3][0::2]):.4f} right {rms(from_left[3][1::2]):.4f}")
    assert rms(last[1::2]) > rms(last[0::2]) > 0.0
    assert rms(from_left[3][0::2]) > rms(from_left[3][1::2]) > 0.0
    swapped = run(mirrored, (0.0, -1.0, 0.0))
    assert np.array_equal(swapped[:, 0::2], from_right[:, 1::2]) and np.array_equal(swapped[:, 1::2], from_right[:, 0::2])


# ---- contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_single_and_permuted_agree(pkg):
    """sources of 1, 3 and 8 slots with 0, 1 and 5 entries (rotating) in one batch of stride 5"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(3)
    frame, taps, n = 320, 15, 3
    dirs, hrir = make_set(pkg, 258, 7, rng)
    ctx.hrtf_set(dirs, hrir)
    V = [1, 3, 8]
    sets = [[ctx.create_source() for _ in range(n)] for _ in range(3)]   # one call | three calls | permuted order
    for group in sets:
        for s, v in zip(group, V):
            ctx.binaural_render_init(s, frame, taps, v, 0.02)
    models = [Model(table_of(pkg, ctx, taps), dirs, hrir, frame, v) for v in V]
    perm = [2, 0, 1]
    counts = [[0, 1, 5], [1, 5, 0], [5, 0, 1], [1, 1, 5]]
    for cb in range(4):
        blk = noise(rng, n, frame)
        lists = [[entry(50 + k, rng.uniform(0, 600), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(counts[cb][i])]
                 for i in range(n)]
        out, mix, rows = ctx.binaural_render_process_batch(sets[0], blk, lists, stride=5, want_mix=True)
        singles = [one(ctx, sets[1][i], blk[i], lists[i], stride=5) for i in range(n)]
        pout, pmix, prows = ctx.binaural_render_process_batch([sets[2][i] for i in perm], blk[perm], [lists[i] for i in perm], stride=5,
                                                              want_mix=True)
        for i in range(n):
            want = models[i].process(blk[i], lists[i])
            assert_same((out[i], tuple(int(x) for x in rows[i])), want, f"batch {cb} {i}")
            assert_same(singles[i], want, f"single {cb} {i}")
            j = perm.index(i)
            assert_same((pout[j], tuple(int(x) for x in prows[j])), want, f"permuted {cb} {i}")
        assert mix.tobytes() == mix_model(out).tobytes(), "mix is not the fp32 sum in list order"
        assert pmix.tobytes() == mix_model(pout).tobytes()
    blk2 = noise(rng, n, frame)   # with out == NULL only the mix comes back; the state moves on all the same
    only_mix, rows2 = ctx.binaural_render_process_batch(sets[0], blk2, lists, stride=5, want_out=False, want_mix=True)
    wants = [models[i].process(blk2[i], lists[i]) for i in range(n)]
    assert only_mix.shape == (2 * frame,) and only_mix.tobytes() == mix_model([w[0] for w in wants]).tobytes()
    assert [tuple(int(x) for x in r) for r in rows2] == [w[1] for w in wants]
    for s in sum(sets, []):
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    cap = pkg._capi
    lib = cap.load()
    ctx = pkg.Context(num_bands=3)
    rng = np.random.default_rng(5)
    frame, taps = 64, 15
    dirs, hrir = make_set(pkg, 6, 7, rng)
    uninit_early = ctx.create_source()
    assert lib.fs_binaural_render_init(ctx.h, uninit_early, frame, taps, 3, C.c_float(0.01)) == cap.ERR_INVALID_ARGUMENT, "no set in force"
    assert ctx.hrtf_info() == (0, 0)
    ctx.hrtf_set(dirs, hrir)
    srcs = [ctx.create_source() for _ in range(3)]
    for s, v in zip(srcs, (2, 3, 4)):
        ctx.binaural_render_init(s, frame, taps, v, 0.01)   # D = 480
    other_frame, other_taps, uninit, dead = (ctx.create_source() for _ in range(4))
    ctx.binaural_render_init(other_frame, 128, taps, 3, 0.01)
    ctx.binaural_render_init(other_taps, frame, 31, 3, 0.01)
    ctx.binaural_render_init(dead, frame, taps, 3, 0.01)
    ctx.reflection_render_init(uninit, frame, taps, 3, 0.01)   # (another renderer's state is not this one's)
    ctx.destroy_source(dead)
    models = [Model(table_of(pkg, ctx, taps), dirs, hrir, frame, v) for v in (2, 3, 4)]
    gains = np.full(8, 0.5, np.float32)

    def good_call():
        blk = noise(rng, 3, frame)
        lists = [[entry(k, rng.uniform(0, 400), gains, 0.5, rng.normal(size=3)) for k in range(2)] for _ in range(3)]
        out, rows = ctx.binaural_render_process_batch(srcs, blk, lists)
        for i in range(3):
            assert_same((out[i], tuple(int(x) for x in rows[i])), models[i].process(blk[i], lists[i]), f"source {i}")

    good_call()
    blk = noise(rng, 3, frame)
    sentinel = np.full((3, 2 * frame), 7.0, np.float32)
    out, mix = sentinel.copy(), sentinel[0].copy()
    rows = np.full((3, 4), 7, np.uint32)
    inf, nan = float("inf"), float("nan")
    base = np.zeros((3, 2), dtype=pkg.Context.BINAURAL_VOICE_DTYPE)
    for i in range(3):
        for e in range(2):
            base[i, e] = (e, 0.001 * (i + e + 1), gains, 0.5, (0.0, 1.0, 0.5))

    def call(sources=srcs, count=3, table=base, counts=(2, 2, 2), stride=2, blocks=blk, dest=out, mixed=None, voices=True, cnts=True, handles=True):
        arr = (C.c_int32 * len(sources))(*sources)
        t = np.ascontiguousarray(table)
        n = np.asarray(counts, np.int32)
        return lib.fs_binaural_render_process_batch(ctx.h, arr if handles else None, count, blocks.ctypes.data if blocks is not None else None,
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
    wide = np.zeros((3, 33), dtype=pkg.Context.BINAURAL_VOICE_DTYPE)
    for stride, table in ((0, base), (-1, base), (33, wide)):
        assert call(stride=stride, table=table, counts=(0, 0, 0)) == cap.ERR_INVALID_ARGUMENT, stride
    assert call(table=with_entry("key", 0)) == cap.ERR_INVALID_ARGUMENT, "a key twice in one row"
    for v in (-0.001, nan, inf, 481.0 / FS):
        assert call(table=with_entry("delay", v)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (-0.5, nan, inf):
        assert call(table=with_entry("band_gain", v, 1)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (nan, inf, -inf):
        assert call(table=with_entry("gain", v)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (nan, inf, -inf):   # a bad direction
        for axis in range(3):
            assert call(table=with_entry("direction", v, axis)) == cap.ERR_INVALID_ARGUMENT, (v, axis)
    assert call(table=with_entry("direction", (0.0, -0.0, 0.0))) == cap.ERR_INVALID_ARGUMENT, "the zero vector has no direction"
    for count in (0, -1, 257):
        assert call(count=count) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], srcs[1], srcs[0]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_frame, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_taps, srcs[2]]) == cap.ERR_INVALID_ARGUMENT, "sources whose T differ"
    assert call(sources=[srcs[0], uninit, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], dead, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[srcs[0], 12345, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[-1, srcs[1], srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(handles=False) == cap.ERR_INVALID_ARGUMENT
    assert call(blocks=None) == cap.ERR_INVALID_ARGUMENT
    assert call(voices=False) == cap.ERR_INVALID_ARGUMENT
    assert call(cnts=False) == cap.ERR_INVALID_ARGUMENT
    assert call(dest=None) == cap.ERR_INVALID_ARGUMENT, "out == NULL && mix == NULL"
    assert call(table=with_entry("direction", nan, 0), mixed=mix) == cap.ERR_INVALID_ARGUMENT

    # refused sets: nothing changes, the held voices go on
    desc = cap.HrtfDesc(C.sizeof(cap.HrtfDesc), 6, 7, FS, dirs.ctypes.data, hrir.ctypes.data)

    def set_with(**kw):
        d = cap.HrtfDesc(desc.struct_size, desc.directions, desc.taps, desc.sample_rate, desc.dirs, desc.hrir)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.fs_hrtf_set(ctx.h, C.byref(d))

    long_dirs, nan_dirs, nan_hrir = dirs.copy(), dirs.copy(), hrir.copy()
    long_dirs[4] *= F32(1.001)   # squared length 1.002
    nan_dirs[5, 1] = nan
    nan_hrir[3, 1, 6] = inf
    wide_dirs, wide_hrir = np.tile(dirs[:1], (4097, 1)), np.zeros((4097, 2, 1), np.float32)
    long_hrir = np.zeros((6, 2, 513), np.float32)
    for kw in (dict(struct_size=desc.struct_size - 4), dict(directions=0), dict(directions=-1), dict(taps=0), dict(sample_rate=FS + 1),
               dict(dirs=None), dict(hrir=None), dict(dirs=long_dirs.ctypes.data), dict(dirs=nan_dirs.ctypes.data), dict(hrir=nan_hrir.ctypes.data),
               dict(directions=4097, taps=1, dirs=wide_dirs.ctypes.data, hrir=wide_hrir.ctypes.data), dict(taps=513, hrir=long_hrir.ctypes.data)):
        assert set_with(**kw) == cap.ERR_INVALID_ARGUMENT, kw
    assert ctx.hrtf_info() == (6, 7)
    assert np.array_equal(out, sentinel) and np.array_equal(mix, sentinel[0]) and np.all(rows == 7), "a refused call wrote"
    good_call()   # every refused call left all three sources and the set as they were: nothing started anew
    blk = noise(rng, 3, frame)
    assert call(table=with_entry("band_gain", nan, 3), blocks=blk) == cap.OK, "entries beyond num_bands are ignored"
    for i in range(3):   # (that call was a callback like any other)
        lst = [(int(base[i, e]["key"]), float(base[i, e]["delay"]), gains, 0.5, (0.0, 1.0, 0.5)) for e in range(2)]
        assert_same((out[i], tuple(int(x) for x in rows[i])), models[i].process(blk[i], lst), f"source {i}")

    # init refusals; a refused init leaves the source as it was
    for args in ((15, 15, 3, 0.01), (16385, 15, 3, 0.01), (frame, 16, 3, 0.01), (frame, 0, 3, 0.01), (frame, 2049, 3, 0.01), (frame, 2043, 3, 0.01),
                 (frame, taps, 0, 0.01), (frame, taps, -1, 0.01), (frame, taps, 33, 0.01), (frame, taps, 3, -0.01), (frame, taps, 3, nan),
                 (frame, taps, 3, inf), (frame, taps, 3, 22.0)):
        assert lib.fs_binaural_render_init(ctx.h, srcs[0], args[0], args[1], args[2], C.c_float(args[3])) == cap.ERR_INVALID_ARGUMENT, args
    assert lib.fs_binaural_render_init(ctx.h, 12345, frame, taps, 3, C.c_float(0.01)) == cap.ERR_BAD_HANDLE
    assert lib.fs_binaural_render_release(ctx.h, 12345) == cap.ERR_BAD_HANDLE
    assert lib.fs_binaural_render_release(ctx.h, uninit) == cap.OK
    good_call()

    # a missing set: the call is refused and nothing is written; the set's return starts the voices anew on the kept history
    ctx.hrtf_set(None, None)
    assert ctx.hrtf_info() == (0, 0)
    assert call() == cap.ERR_INVALID_ARGUMENT, "a missing set"
    assert lib.fs_binaural_render_init(ctx.h, uninit, frame, taps, 3, C.c_float(0.01)) == cap.ERR_INVALID_ARGUMENT
    ctx.hrtf_set(dirs, hrir)
    for m in models:
        m.set(dirs, hrir)
    good_call()
    # a set that outgrows an initialised source's ring: D + Tc + 1 + F = 480 + (15 + 512 - 1) + 1 + 64 > 1024
    ctx.hrtf_set(dirs, np.zeros((6, 2, 512), np.float32))
    assert call() == cap.ERR_INVALID_ARGUMENT
    ctx.hrtf_set(dirs, hrir)
    for m in models:
        m.set(dirs, hrir)
    good_call()
    ctx.close()


@pytest.mark.gpu
def test_a_new_set_starts_every_voice_from_silence(pkg):
    """fs_hrtf_set with voices held: the next callback reports them all as started.  They fade in from silence on the kept history
    with their delays and band gains at their targets, so in exact arithmetic that callback is a(s) times what the same voices
    give held steadily on the new set (source B on a second context that had the new set all along, fed the same blocks): both are
    within bound64 of their exact values, so |A - a B| <= (1 + a) bound <= 2 bound, and no sample of A exceeds B's by more"""
    rng = np.random.default_rng(9)
    frame, taps, H, K = 64, 15, 7, 3
    dirs, old = make_set(pkg, 6, H, rng)
    _, new = make_set(pkg, 6, H, rng)
    ctx_a, ctx_b = pkg.Context(num_bands=3), pkg.Context(num_bands=3)
    ctx_a.hrtf_set(dirs, old)
    ctx_b.hrtf_set(dirs, new)
    a, b = ctx_a.create_source(), ctx_b.create_source()
    ctx_a.binaural_render_init(a, frame, taps, 4, 0.02)
    ctx_b.binaural_render_init(b, frame, taps, 4, 0.02)
    m = Model(table_of(pkg, ctx_a, taps), dirs, old, frame, 4)
    entries = [entry(k, rng.uniform(0, 300), rng.uniform(0, 1, 8), rng.uniform(0.3, 1.0) * (-1) ** k, rng.normal(size=3)) for k in range(K)]
    for cb in range(3):
        blk = noise(rng, 1, frame)[0]
        if cb == 2:
            ctx_a.hrtf_set(dirs, new)
            m.set(dirs, new)
        got = one(ctx_a, a, blk, entries)
        steady = one(ctx_b, b, blk, entries)
        want = m.process(blk, entries, want64=(cb == 2))
        assert_same(got, want[:2], f"callback {cb + 1}")
    assert got[1] == (K, K, 0, 0) and steady[1] == (K, 0, 0, 0)
    bound = bound64(taps, H, 3, K, want[3], want[4])
    ramp = np.repeat(((np.arange(frame) + 1).astype(np.float32) / F32(frame)).astype(np.float64), 2)
    A, B = got[0].astype(np.float64), steady[0].astype(np.float64)
    print(f"a new set: |A - a B| at most {np.abs(A - ramp * B).max() / (2 * bound):.3f} of the bound")
    assert np.all(np.abs(A - ramp * B) <= 2 * bound)
    assert np.all(np.abs(A) <= np.abs(B) + 2 * bound)
    assert np.abs(B).max() > 1000 * bound
    ctx_a.close()
    ctx_b.close()


@pytest.mark.gpu
def test_release_and_reinit(pkg):
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(8)
    dirs, hrir = make_set(pkg, 6, 7, rng)
    ctx.hrtf_set(dirs, hrir)
    src = ctx.create_source()
    frame, taps, V = 64, 15, 3
    ctx.binaural_render_init(src, frame, taps, V, 0.02)
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    entries = [entry(1, 50.5, g[0], 1.0, (0.0, 1.0, 0.2)), entry(2, 300.0, g[1], -0.5, (1.0, -1.0, 0.0))]
    for _ in range(2):
        one(ctx, src, noise(rng, 1, frame)[0], entries)
    ctx.binaural_render_release(src)   # zero history, every slot free: the same keys fade in from silence
    m = Model(table_of(pkg, ctx, taps), dirs, hrir, frame, V)
    for cb in range(2):
        blk = noise(rng, 1, frame)[0]
        got = one(ctx, src, blk, entries)
        assert got[1] == (2, 2 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"after release, callback {cb + 1}")
    for frame, taps, V in ((320, 15, 1), (64, 255, 5)):   # another F, another T, another V — with voices held
        ctx.binaural_render_init(src, frame, taps, V, 0.02)
        m = Model(table_of(pkg, ctx, taps), dirs, hrir, frame, V)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"{(frame, taps, V)} callback {cb + 1}")
    ctx.destroy_source(src)   # with voices held
    other = ctx.create_source()
    ctx.binaural_render_init(other, 64, 15, 2, 0.02)
    m = Model(table_of(pkg, ctx, 15), dirs, hrir, 64, 2)
    blk = noise(rng, 1, 64)[0]
    assert_same(one(ctx, other, blk, entries), m.process(blk, entries), "a new source after the destroy")
    ctx.destroy_source(other)
    closing = pkg.Context(num_bands=1)   # fs_context_destroy with a set, a source and held voices
    closing.hrtf_set(dirs, hrir)
    s = closing.create_source()
    closing.binaural_render_init(s, 64, 15, 2, 0.02)
    one(closing, s, blk, entries)
    closing.close()


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    ctx = pkg.Context(num_bands=3)
    rng = np.random.default_rng(40)
    ctx.hrtf_set(*make_set(pkg, 258, 32, rng))
    frame, taps, n = 64, 15, 40
    srcs = [ctx.create_source() for _ in range(n)]
    for s in srcs:
        ctx.binaural_render_init(s, frame, taps, 4, 0.01)
    blk = noise(rng, n, frame)
    lists = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.0)) for k in range(3)]] * n
    ctx.binaural_render_process_batch(srcs, blk, lists[:n], stride=4, want_mix=True)
    free0 = device_free_bytes()
    for cb in range(20):
        more = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.1 * cb)) for k in range(cb % 2, 4)]] * n   # slots fill up and turn over
        ctx.binaural_render_process_batch(srcs, blk, more, stride=4, want_mix=True)
    ctx.binaural_render_process_batch(srcs[:7], blk[:7], lists[:7], stride=3)   # a smaller shape fits what is there
    assert device_free_bytes() >= free0
    ctx.close()


@pytest.mark.gpu
def test_staging_is_its_own(pkg):
    """one "audio callback" = a reverb batch of 2, a direct batch of 5, a reflection batch of 3 and a binaural batch of 4, three
    rounds; each equals what it gives alone"""
    frame, taps = 1024, 15
    rng = np.random.default_rng(77)
    irs = [noise_ir(rng, 48000) for _ in range(2)]
    the_set = make_set(pkg, 6, 7, rng)
    rev_blocks = [noise(rng, 2, frame) * F32(0.3) for _ in range(3)]
    dir_blocks = [noise(rng, 5, frame) for _ in range(3)]
    ref_blocks = [noise(rng, 3, frame) for _ in range(3)]
    bin_blocks = [noise(rng, 4, frame) for _ in range(3)]
    tg = [[(float(F32(rng.uniform(0, 400) / FS)), rng.uniform(0, 1, 8).astype(np.float32)) for _ in range(5)] for _ in range(3)]
    ref_lists = [[[(k, secs(rng.uniform(0, 400)), rng.uniform(0, 1, 8).astype(np.float32), rng.uniform(-1, 1, 2).astype(np.float32))
                   for k in range(2 + cb)] for _ in range(3)] for cb in range(3)]
    bin_lists = [[[entry(k, rng.uniform(0, 400), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(1 + cb)]
                  for _ in range(4)] for cb in range(3)]

    def run(reverb, direct, reflect, binaural):
        ctx = pkg.Context(num_bands=1)
        ctx.hrtf_set(*the_set)
        rs = [ctx.create_source() for _ in range(2)]
        ds = [ctx.create_source() for _ in range(5)]
        es = [ctx.create_source() for _ in range(3)]
        bs = [ctx.create_source() for _ in range(4)]
        for s, ir in zip(rs, irs):
            ctx.reverb_init(s, frame)
            ctx.set_impulse_response(s, ir)
        for s in ds:
            ctx.direct_render_init(s, frame, taps, 0.01)
        for s in es:
            ctx.reflection_render_init(s, frame, taps, 4, 0.01)
        for s in bs:
            ctx.binaural_render_init(s, frame, taps, 4, 0.01)
        outs = {"reverb": [], "direct": [], "reflect": [], "binaural": []}
        for cb in range(3):
            if reverb:
                outs["reverb"].append(ctx.reverb_process_batch(rs, rev_blocks[cb]).tobytes())
            if direct:
                outs["direct"].append(ctx.direct_render_process_batch(ds, dir_blocks[cb], tg[cb]).tobytes())
            if reflect:
                out, rows = ctx.reflection_render_process_batch(es, ref_blocks[cb], ref_lists[cb])
                outs["reflect"].append(out.tobytes() + rows.tobytes())
            if binaural:
                out, rows = ctx.binaural_render_process_batch(bs, bin_blocks[cb], bin_lists[cb])
                outs["binaural"].append(out.tobytes() + rows.tobytes())
        ctx.close()
        return outs

    together = run(True, True, True, True)
    assert together["reverb"] == run(True, False, False, False)["reverb"], "the reverb rows changed beside the other batches"
    assert together["direct"] == run(False, True, False, False)["direct"], "the direct rows changed beside the other batches"
    assert together["reflect"] == run(False, False, True, False)["reflect"], "the reflection rows changed beside the other batches"
    assert together["binaural"] == run(False, False, False, True)["binaural"], "the binaural rows changed beside the other batches"


@pytest.mark.gpu
def test_one_source_holds_three_renderers(pkg):
    """direct, reflection and binaural state side by side on ONE source: each renderer's output is what a source of its own gives"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(12)
    frame, taps = 64, 15
    dirs, hrir = make_set(pkg, 6, 7, rng)
    ctx.hrtf_set(dirs, hrir)
    both, alone = ctx.create_source(), ctx.create_source()
    ctx.direct_render_init(both, frame, taps, 0.02)
    ctx.reflection_render_init(both, frame, taps, 2, 0.02)
    ctx.binaural_render_init(both, frame, taps, 2, 0.02)
    ctx.binaural_render_init(alone, frame, taps, 2, 0.02)
    g = rng.uniform(0, 1, 8).astype(np.float32)
    for cb in range(3):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(1, 90.0 + 7.3 * cb, g, 0.8, rng.normal(size=3))]
        ctx.direct_render_process_batch([both], blk[None], [(secs(50.0), g)])
        ctx.reflection_render_process_batch([both], blk[None], [[(3, secs(70.0), g, (0.5, 0.5))]])
        assert_same(one(ctx, both, blk, entries), one(ctx, alone, blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(both)
    ctx.destroy_source(alone)


@pytest.mark.gpu
def test_component_layer(pkg):
    """UpdateDirectPaths + UpdateReflectionPaths -> FrequenSeeAudioBinauralPlugin.ProcessAudio in the 12-triangle shoebox, the
    listener facing +x with the right ear to +y, the source moving past 100 cm to its right: while it
    is on the right, the direct voice alone — Voices() with no reflection — is louder in the right ear; and the plugin's call with
    every voice equals the C call with Voices()' entries"""
    w = shoebox_world()
    frame, taps = 256, 15
    fwd, right = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]

    def world():
        sub = pkg.AudioRayTracingSubsystem(num_bands=4)
        sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
        sub.SetMaterials(w.absorption, w.transmission, w.scattering)
        comp = pkg.FrequenSeeAudioComponent(SRC)
        comp.OnRegister(sub)
        sub.SetListenerLocation(LIS)
        return sub, comp

    sub, comp = world()
    plug = pkg.FrequenSeeAudioBinauralPlugin(sub)
    plug.Initialize(frame, taps, 16, 0.05)
    plug.SetHrtf(directions=258, taps=64)
    assert sub.ctx.hrtf_info() == (258, 64)
    plug.OnInitSource(comp)
    sub2, comp2 = world()
    sub2.ctx.hrtf_set(*pkg.Context.hrtf_spherical_head(FS, 258, 64))
    sub2.ctx.binaural_render_init(comp2._src, frame, taps, 16, 0.05)
    sub3, comp3 = world()   # the direct voice alone
    sub3.ctx.hrtf_set(*pkg.Context.hrtf_spherical_head(FS, 258, 64))
    sub3.ctx.binaural_render_init(comp3._src, frame, taps, 2, 0.05)
    empty_row = np.zeros(1, dtype=pkg.Context.REFLECTION_ROW_DTYPE)[0]
    rng = np.random.default_rng(2)
    lis = np.asarray(LIS, np.float64)
    direct_out = []
    for cb, dx in enumerate((-60.0, -20.0, 20.0, 60.0)):   # past the listener, 100 cm to its right
        pos = [float(lis[0] + dx), float(lis[1] + 100.0), float(lis[2])]
        comp.SetComponentLocation(pos)
        direct = sub.UpdateDirectPaths()
        rows, paths = sub.UpdateReflectionPaths(max_paths=8)
        mono = np.repeat(rng.uniform(-1.0, 1.0, frame).astype(np.float32), 2)[None]
        got, grow = plug.ProcessAudio([comp], mono, rows, paths, fwd, right, reference_length=500.0, direct=(direct, LIS))
        voices = plug.Voices(rows[0], paths[0], fwd, right, 500.0, direct=(direct[0], np.asarray(pos) - lis))
        assert voices.shape == (1 + int(rows[0]["returned"]),) and int(voices["key"][0]) == DIRECT_KEY
        assert np.array_equal(voices["key"][1:], paths[0]["triangle"][:int(rows[0]["returned"])])
        assert voices["direction"][0][1] > 0.0, "the source is on the right"
        want, wrow = sub2.ctx.binaural_render_process_batch([comp2._src], mono, [voices])
        assert int(grow[0]["dropped"]) == 0
        assert got.tobytes() == want.tobytes() and grow.tobytes() == wrow.tobytes()
        only = plug.Voices(empty_row, paths[0], fwd, right, 500.0, direct=(direct[0], np.asarray(pos) - lis))
        assert only.shape == (1,)
        direct_out.append(sub3.ctx.binaural_render_process_batch([comp3._src], mono, [only])[0][0])
    heard = np.concatenate(direct_out[1:])   # (the first block fades in)
    rms_left, rms_right = (float(np.sqrt(np.mean(heard[ch::2].astype(np.float64) ** 2))) for ch in range(2))
    print(f"the direct voice passing on the right: rms left {rms_left:.4f} right {rms_right:.4f}")
    assert rms_right > rms_left > 0.0
    plug.OnReleaseSource(comp)
    for s in (sub, sub2, sub3):
        s.Deinitialize()
