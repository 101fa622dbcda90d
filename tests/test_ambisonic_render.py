"""fs_ambisonic_render_process_batch: every discrete path of a source rendered into an ambisonic bus — the reflection renderer's
voice bank on ONE mono history (the block's downmix), each voice evaluated once and fanned out to the C = (order + 1)^2 channels
(ACN order, SN3D normalisation, orders 0 .. 3) by ramping gains g * Y_c(direction) (include/frequensee.h, "ambisonic voices on the
audio thread").

Yardsticks.  For the encoding: the real spherical harmonics from their definition — sqrt((2 - delta_m0) (n - |m|)! / (n + |m|)!)
P_n^|m|(z) {cos, sin}(|m| az), no Condon-Shortley phase, the Legendre polynomials from numpy.polynomial.legendre — in float64 under
a bound derived from the operation count, and a numpy float32 restatement of the header's formulas which fs_ambisonic_encode must
EQUAL.  For the callback: Model below, a numpy float32 restatement of the header's rule which the device must EQUAL (tobytes()),
itself held against the same rule in float64 with the float64 definition of the encoding; and a yardstick this code did not
write, the reflection renderer on the device, which any pair of channels must equal to the bit when it is fed g * Y_c as channel
gains.  Then known answers that need no restatement, and the batch, state and refusal rules.
"""
import ctypes as C
from math import factorial

import numpy as np
import pytest
from numpy.polynomial import legendre

from test_direct_paths import device_free_bytes
from test_direct_render import EPS, F32, FS
from test_direct_render import _close_contexts  # noqa: F401  (closes the contexts ctx_for caches when this module is done)
from test_direct_render import ctx_for, mix_model, noise, table_of, taps32
from test_reflection_paths import LIS, SRC, shoebox_world
from test_reflection_render import bank_schedule, secs

MAX_VOICES = 32
MAX_ORDER = 3


def channels(order):
    return (order + 1) ** 2


# ---- the encoding --------------------------------------------------------------------------------------------------------------
K3, K3H, K58 = F32(np.sqrt(3.0)), F32(np.sqrt(3.0) / 2), F32(np.sqrt(5.0 / 8))
K15, K38, K15H = F32(np.sqrt(15.0)), F32(np.sqrt(3.0 / 8)), F32(np.sqrt(15.0) / 2)


def len2_32(d):
    d = np.asarray(d, np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def encode32(order, d):
    """the header's formulas in numpy float32, every operation in the order written: d [..., 3] -> [..., C]"""
    d = np.asarray(d, np.float32)
    ln = np.sqrt(len2_32(d))
    x, y, z = d[..., 0] / ln, -(d[..., 1] / ln), d[..., 2] / ln
    xx, yy, zz = x * x, y * y, z * z
    one = np.ones_like(x)
    Y = [one,
         y, z, x,
         K3 * (x * y), K3 * (y * z), F32(1.5) * zz - F32(0.5), K3 * (x * z), K3H * (xx - yy),
         K58 * (y * (F32(3.0) * xx - yy)), K15 * ((x * y) * z), K38 * (y * (F32(5.0) * zz - F32(1.0))), z * (F32(2.5) * zz - F32(1.5)),
         K38 * (x * (F32(5.0) * zz - F32(1.0))), K15H * (z * (xx - yy)), K58 * (x * (xx - F32(3.0) * yy))]
    out = np.stack([np.asarray(v, np.float32) for v in Y[:channels(order)]], axis=-1)
    assert out.dtype == np.float32 and all(np.asarray(v).dtype == np.float32 for v in Y)
    return out


def encode64(order, d):
    """the definition, in float64, of float32 directions d [..., 3] in the head frame (x forward, y right, z up; AmbiX's y is to
    the left): channel n (n + 1) + m is sqrt((2 - delta_m0) (n - |m|)! / (n + |m|)!) P_n^|m|(z) cos(m az) for m >= 0 and
    ... sin(|m| az) for m < 0, P_n^m(z) = (1 - z^2)^(m / 2) d^m/dz^m P_n(z) (no Condon-Shortley phase)"""
    d = np.asarray(d, np.float32).astype(np.float64)
    ln = np.sqrt((d ** 2).sum(axis=-1))
    x, y, z = d[..., 0] / ln, -d[..., 1] / ln, d[..., 2] / ln
    az = np.arctan2(y, x)
    rho = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    out = np.zeros(d.shape[:-1] + (channels(order),))
    for n in range(order + 1):
        for m in range(-n, n + 1):
            am = abs(m)
            P = legendre.Legendre.basis(n).deriv(am)(z) * rho ** am if am else legendre.Legendre.basis(n)(z)
            norm = np.sqrt((1.0 if m == 0 else 2.0) * factorial(n - am) / factorial(n + am))
            out[..., n * (n + 1) + m] = norm * P * (np.cos(am * az) if m >= 0 else np.sin(am * az))
    return out


# |Y32 - Y64| for a channel of order <= 3, u = 2^-24, derived:
#  - the normalisation.  The squared length is three rounded products of positive terms and two rounded sums, (1 + u)^3; the square
#    root halves that and rounds, the division rounds: every component (|.| <= 1) is off by at most 3.5 u.  The polynomial moves by
#    at most that times the sum of the absolute values of its partial derivatives on the unit sphere, G <= 6: the worst is
#    Y12 = z (2.5 zz - 1.5) with |7.5 zz - 1.5| <= 6; Y11 / Y13: K38 (|5 zz - 1| + 10 |y z|) <= 5.6; Y14: K15h (|xx - yy| + 2 |z| (|x| + |y|))
#    <= 4.7; Y10: K15 (|yz| + |xz| + |xy|) <= 3.9; Y9 / Y15: K58 (6 |xy| + 3 |xx - yy|) <= 3.4; orders 1 and 2 less.
#  - the evaluation.  At most 6 roundings per channel (Y9: xx, yy, 3 xx, the difference, the product with y, the product with K58), and
#    every rounded intermediate times the factors still to come is at most 4 in magnitude (5 zz |y| K38 <= 3.1, 3 xx |y| K58 <= 2.4,
#    2.5 zz |z| <= 2.5): 4 u each.
#  - the constant, rounded to float once: u |Y| <= u.
G_MAX = 6.0
ENCODE_BOUND = (6 * 4.0 + G_MAX * 3.5 + 1.0) * EPS   # 46 u = 2.74e-6

AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)


def directions(rng, n):
    """n random directions of lengths from 1e-3 to 1e3, then the axes"""
    d = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return np.concatenate([d.astype(np.float32), AXES, AXES * F32(7.5)])


def encode_all(pkg, order, dirs):
    return np.stack([pkg.Context.ambisonic_encode(order, d) for d in dirs])


def test_struct_and_exports(pkg):
    cap = pkg._capi
    assert cap.AmbisonicVoice is cap.BinauralVoice and C.sizeof(cap.AmbisonicVoice) == 56 and C.sizeof(cap.AmbisonicRenderRow) == 16
    R = cap.AmbisonicRenderRow
    assert (R.sounding.offset, R.started.offset, R.ended.offset, R.dropped.offset) == (0, 4, 8, 12)
    assert pkg.Context.AMBISONIC_VOICE_DTYPE.itemsize == 56 and pkg.Context.AMBISONIC_RENDER_ROW_DTYPE.itemsize == 16
    assert cap.MAX_AMBISONIC_ORDER == MAX_ORDER
    for name in ("fs_ambisonic_encode", "fs_ambisonic_render_init", "fs_ambisonic_render_release", "fs_ambisonic_render_process_batch"):
        assert name in cap.EXPORTS and hasattr(cap.load(), name)
    assert cap.load().fs_abi_version() == 5
    assert issubclass(pkg.FrequenSeeAudioAmbisonicPlugin, pkg.FrequenSeeAudioBinauralPlugin)
    assert pkg.FrequenSeeAudioAmbisonicPlugin.Order == 1
    assert pkg.FrequenSeeAudioAmbisonicPlugin.Voices is pkg.FrequenSeeAudioBinauralPlugin.Voices, "Voices() is inherited unchanged"


def test_encode_against_the_definition(pkg):
    """fs_ambisonic_encode against encode64 within ENCODE_BOUND, derived above: orders 0 .. 3, 3000 random directions of many
    lengths and the axes; the worst observed share of the bound is printed"""
    rng = np.random.default_rng(0xA3B1)
    dirs = directions(rng, 3000)
    worst = 0.0
    for order in range(MAX_ORDER + 1):
        got = encode_all(pkg, order, dirs)
        assert got.shape == (dirs.shape[0], channels(order)) and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - encode64(order, dirs)).max()
        worst = max(worst, float(err / ENCODE_BOUND))
        assert err <= ENCODE_BOUND, (order, err)
    print(f"encode vs the definition: worst share of the bound {worst:.3f} (bound {ENCODE_BOUND:.3e})")
    assert np.abs(encode64(3, dirs)).max() <= 1.0 + 1e-12, "|Y_c| <= 1 under SN3D"


def test_encode_known_answers(pkg):
    """a voice straight ahead (+x), to the left (-y in the head frame: AmbiX +y) and above (+z), by value"""
    e = pkg.Context.ambisonic_encode
    ahead, left, above = e(3, (2.0, 0.0, 0.0)), e(3, (0.0, -0.5, 0.0)), e(3, (0.0, 0.0, 4.0))
    assert list(ahead[:4]) == [1.0, 0.0, 0.0, 1.0] and ahead[6] == -0.5 and ahead[8] == K3H and ahead[15] == K58 and ahead[13] == -K38
    assert list(left[:4]) == [1.0, 1.0, 0.0, 0.0] and left[6] == -0.5 and left[8] == -K3H and left[9] == -K58 and left[11] == -K38
    assert list(above[:4]) == [1.0, 0.0, 1.0, 0.0] and above[6] == 1.0 and above[12] == 1.0
    assert not above[[1, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 15]].any()


def test_encode_equals_the_float32_restatement(pkg):
    rng = np.random.default_rng(0xA3B2)
    dirs = directions(rng, 3000)
    for order in range(MAX_ORDER + 1):
        assert encode_all(pkg, order, dirs).tobytes() == encode32(order, dirs).tobytes(), order


def test_each_orders_squares_sum_to_one(pkg):
    """per order n and direction, sum_m Y_nm^2 = 1 (SN3D), the squares summed in float64, within ENCODE_BOUND"""
    rng = np.random.default_rng(0xA3B3)
    dirs = directions(rng, 3000)
    Y = encode_all(pkg, MAX_ORDER, dirs).astype(np.float64)
    worst = 0.0
    for n in range(MAX_ORDER + 1):
        total = (Y[:, n * n:(n + 1) * (n + 1)] ** 2).sum(axis=1)
        worst = max(worst, float(np.abs(total - 1.0).max() / ENCODE_BOUND))
        assert np.all(np.abs(total - 1.0) <= ENCODE_BOUND), n
    print(f"sum of squares per order: worst share of the bound {worst:.3f}")


def test_encode_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    out = np.full(16, 7.0, np.float32)

    def call(order, d, dest=out):
        a = None if d is None else np.asarray(d, np.float32)
        return lib.fs_ambisonic_encode(order, None if a is None else a.ctypes.data, None if dest is None else dest.ctypes.data)

    inf, nan = float("inf"), float("nan")
    for order in (-1, 4, 100):
        assert call(order, (1.0, 0.0, 0.0)) == cap.ERR_INVALID_ARGUMENT, order
    assert call(1, None) == cap.ERR_INVALID_ARGUMENT and call(1, (1.0, 0.0, 0.0), None) == cap.ERR_INVALID_ARGUMENT
    for d in ((0.0, 0.0, 0.0), (0.0, -0.0, 0.0), (nan, 0.0, 1.0), (1.0, inf, 0.0), (1.0, 0.0, -inf),
              (1e-16, 0.0, 0.0),       # squared length 1e-32, below 1e-30
              (1e-20, 1e-20, 1e-20),   # ... 0 after underflow
              (2e15, 0.0, 0.0),        # ... 4e30, above 1e30
              (3e19, 3e19, 0.0)):      # ... not finite in fp32, with finite components
        assert call(3, d) == cap.ERR_INVALID_ARGUMENT, d
    assert np.all(out == 7.0), "a refused call wrote"
    for d in ((1.1e-15, 0.0, 0.0), (0.0, 9e14, 0.0), (1e-15, 1e-15, 1e-15)):   # inside the range, close to its ends
        assert F32(1e-30) <= len2_32(d) <= F32(1e30)
        assert call(3, d) == cap.OK, d
        assert out.tobytes() == encode32(3, np.asarray(d, np.float32)).tobytes()
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.ambisonic_encode(4, (1.0, 0.0, 0.0))


def test_null_context_and_null_pointers(pkg):
    cap = pkg._capi
    lib = cap.load()
    src = (C.c_int32 * 1)(0)
    cnt = (C.c_int32 * 1)(1)
    blk = np.zeros(128, np.float32)
    out = np.full(64 * 16, 7.0, np.float32)
    mix = np.full(64 * 16, 7.0, np.float32)
    rows = np.full(4, 7, np.uint32)
    vo = np.zeros(1, dtype=pkg.Context.AMBISONIC_VOICE_DTYPE)
    vo["direction"] = (1.0, 0.0, 0.0)
    a, o, m, v, r = blk.ctypes.data, out.ctypes.data, mix.ctypes.data, vo.ctypes.data, rows.ctypes.data
    call = lib.fs_ambisonic_render_process_batch
    assert lib.fs_ambisonic_render_init(None, 0, 64, 15, 4, 0.01, 1) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_ambisonic_render_release(None, 0) == cap.ERR_INVALID_ARGUMENT
    assert call(None, src, 1, a, v, cnt, 1, o, m, r) == cap.ERR_INVALID_ARGUMENT
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        cfg = cap.default_config(num_bands=1)
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == cap.ERR_NO_DEVICE and h
        try:
            assert lib.fs_ambisonic_render_init(h, 0, 64, 15, 4, 0.01, 1) == cap.ERR_NO_DEVICE
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
def downmix(block):
    block = np.asarray(block, np.float32)
    x = F32(0.5) * (block[0::2] + block[1::2])
    assert x.dtype == np.float32
    return x


class Model:
    """One source's callback, as include/frequensee.h states it.  An entry is (key, delay in s, band gains, gain, direction).
    process() returns (the fp32 output [F][C], the row's counts (sounding, started, ended, dropped)); with want64 also the same rule
    with d, i, f, a from the fp32 rule, the exact downmix, the encoding from its float64 definition and every multiply-accumulate
    in float64, and the two weights of the bound per channel (bound64)."""

    def __init__(self, table, frame, voices, order, fs=FS):
        self.k = np.asarray(table, np.float32)
        self.B, self.T = self.k.shape
        self.F, self.V, self.fs, self.order, self.C = frame, voices, fs, order, channels(order)
        self.release()

    def release(self):
        self.x = np.zeros(0, np.float32)     # x(n) for n >= 0; zero before
        self.x64 = np.zeros(0, np.float64)   # the downmix without its rounding
        self.n0 = 0
        self.slots = [None] * self.V   # None = free, else dict(key, d0, g0, w0, w64, gain)

    def sample(self, x, p):
        return np.where(p >= 0, x[np.maximum(p, 0)], x.dtype.type(0.0)).astype(x.dtype)

    def match(self, entries):
        """rule 1: per slot None or (kind, d0, g0, w0, w0_64, gain0, d1, g1, w1, w1_64, gain1, key), and the counts"""
        plan = [None] * self.V
        started = ended = dropped = 0
        target = {}
        zero, zero64 = np.zeros(self.C, np.float32), np.zeros(self.C, np.float64)
        for key, delay, gains, gain, direction in entries:
            assert key not in target
            w1 = F32(gain) * encode32(self.order, np.asarray(direction, np.float32))
            assert w1.dtype == np.float32 and w1.shape == (self.C,)
            w64 = float(F32(gain)) * encode64(self.order, np.asarray(direction, np.float32))
            target[key] = (F32(delay) * F32(self.fs), np.asarray(gains, np.float32)[:self.B].copy(), w1, w64, abs(float(F32(gain))))
        free = [j for j in range(self.V) if self.slots[j] is None]   # as the callback began
        for j, st in enumerate(self.slots):
            if st is None:
                continue
            held = (st["d0"], st["g0"], st["w0"], st["w64"], st["gain"])
            if st["key"] in target:
                plan[j] = ("continue",) + held + target.pop(st["key"]) + (st["key"],)
            else:
                plan[j] = ("end",) + held + (st["d0"], st["g0"], zero, zero64, 0.0, st["key"])
                ended += 1
        for key, t in target.items():   # (a dict keeps the list order)
            if free:
                plan[free.pop(0)] = ("start", t[0], t[1], zero, zero64, 0.0) + t + (key,)
                started += 1
            else:
                dropped += 1
        return plan, (sum(p is not None for p in plan), started, ended, dropped)

    def process(self, block, entries, want64=False):
        F, T, Cn = self.F, self.T, self.C
        block = np.asarray(block, np.float32)
        plan, row = self.match(entries)
        half = F32(0.5) * F32(F)
        s = np.arange(F)
        a = (s + 1).astype(np.float32) / F32(F)
        a64 = a.astype(np.float64)
        self.x = np.concatenate([self.x, downmix(block)])
        self.x64 = np.concatenate([self.x64, 0.5 * (block[0::2].astype(np.float64) + block[1::2].astype(np.float64))])
        out = np.zeros((F, Cn), np.float32)
        out64 = np.zeros((F, Cn), np.float64)
        weight, weight_gain = np.zeros(Cn), 0.0
        for j, p in enumerate(plan):   # ascending slot number
            if p is None:
                continue
            kind, d0, g0, w0, w0_64, gain0, d1, g1, w1, w1_64, gain1, key = p
            e = np.clip(d1 - d0, -half, half).astype(np.float32)
            c0, c1 = taps32(self.k, g0), taps32(self.k, g1)
            dc = c1 - c0
            d = d0 + a * e
            fl = np.floor(d)
            f = d - fl
            i = fl.astype(np.int64)
            assert a.dtype == d.dtype == f.dtype == dc.dtype == np.float32
            acc = [np.zeros(F, np.float32) for _ in range(4)]
            acc64 = np.zeros(F, np.float64)
            for t in range(T):
                c = c0[t] + a * dc[t]
                q = self.n0 + s - t - i
                xp, xm = self.sample(self.x, q), self.sample(self.x, q - 1)
                v = xp + f * (xm - xp)
                acc[t % 4] = acc[t % 4] + c * v
                if want64:
                    c64 = np.float64(c0[t]) + a64 * (np.float64(c1[t]) - np.float64(c0[t]))
                    xp64, xm64 = self.sample(self.x64, q), self.sample(self.x64, q - 1)
                    acc64 += c64 * (xp64 + f.astype(np.float64) * (xm64 - xp64))
            y = (acc[0] + acc[1]) + (acc[2] + acc[3])
            dw = w1 - w0
            assert y.dtype == dw.dtype == np.float32
            for c in range(Cn):
                w = w0[c] + a * dw[c]
                assert w.dtype == np.float32
                out[:, c] = out[:, c] + w * y
                out64[:, c] += (w0_64[c] + a64 * (w1_64[c] - w0_64[c])) * acc64
            csum = max(np.abs(c0.astype(np.float64)).sum(), np.abs(c1.astype(np.float64)).sum())
            weight += np.maximum(np.abs(w0), np.abs(w1)).astype(np.float64) * csum
            weight_gain += max(gain0, gain1) * csum
            if kind == "end":
                self.slots[j] = None
            else:
                g_after = np.zeros(self.B, np.float32)
                g_after[:] = g1
                self.slots[j] = dict(key=key, d0=F32(d0 + e), g0=g_after, w0=w1.copy(), w64=w1_64.copy(), gain=gain1)
        assert out.dtype == np.float32
        self.n0 += F
        if want64:
            return out, row, out64, weight, weight_gain
        return out, row


def bound64(T, K, weight, weight_gain, peak=1.0):
    """|y - y64| of a channel <= max|x| (2^-24 (T + 10 + K + 2) W + ENCODE_BOUND W_g).
    The first term is the reflection renderer's derived bound, (T + 8 + K + 2) roundings relative to W = sum_j max(|w0_j|, |w1_j|)
    max(sum |c0_j|, sum |c1_j|) — per voice T rounded products and sums plus the coefficient's lerp and the tap interpolation, one
    rounding per product and per sum of the K voices' weighted sum and the gain ramp's two — with two more: the downmix
    0.5f * (l + r) rounds its sum once (the halving is exact), and w1 = g * Y_c rounds its product once.  The second is the
    encoding's own error, at most ENCODE_BOUND in Y_c whatever the channel, times the gain: relative to
    W_g = sum_j max(|g0_j|, |g1_j|) max(sum |c0_j|, sum |c1_j|)."""
    return peak * (EPS * (T + 10 + K + 2) * weight + ENCODE_BOUND * weight_gain)


def entry(key, samples, gains, gain, direction, fs=FS):
    return (key, secs(samples, fs), np.asarray(gains, np.float32), float(F32(gain)), np.asarray(direction, np.float32))


def test_restatement_against_float64(pkg):
    """bound64, derived there, not measured.  40 random cases, K <= 4 voices, every order, L != R, the second callback ramping
    delays, gains and directions; the worst observed share of the bound is printed"""
    rng = np.random.default_rng(0xA3B4)
    worst = 0.0
    for case in range(40):
        bands, taps, frame, K = int(rng.choice([1, 3, 8])), int(rng.choice([15, 63, 255])), 32, int(rng.integers(1, 5))
        m = Model(pkg.Context.direct_band_kernels(FS, bands, taps), frame, K, case % 4)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            entries = [(k, float(rng.uniform(0.0, 300.0)) / FS, rng.uniform(0.0, 1.0, 8), float(rng.uniform(-1.0, 1.0)), rng.normal(size=3))
                       for k in range(K)]
            y, row, y64, weight, weight_gain = m.process(blk, entries, want64=True)
        assert row == (K, 0, 0, 0)
        share = np.abs(y - y64).max(axis=0) / bound64(taps, K, weight, weight_gain)
        worst = max(worst, float(share.max()))
    print(f"restatement vs float64: worst share of the bound {worst:.3f}")
    assert worst <= 1.0


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def one(ctx, src, block, entries, **kw):
    out, rows = ctx.ambisonic_render_process_batch([src], block[None], [entries], **kw)
    return out[0], tuple(int(x) for x in rows[0])


def assert_same(got, want, where):
    (g, grow), (w, wrow) = got, want
    assert grow == wrow, f"{where}: rows {grow} != {wrow}"
    assert g.shape == w.shape, f"{where}: {g.shape} != {w.shape}"
    bad = np.argwhere(g != w)
    assert g.tobytes() == w.tobytes(), f"{where}: {len(bad)} values differ, first at (sample, channel) {bad[:4].tolist()}"


def ambisonic_schedule(rng):
    """the reflection renderer's eight-callback script (bank_schedule: start | steady | ramps, one gain negative | a key vanishing
    while another starts | the key returning in a permuted list | a fourth entry | all ending | silence) with the first channel
    gain as the gain and a random direction per entry: steady over the first two callbacks, then a new one in every callback"""
    fixed = {}
    script = []
    for cb, (entries, counts) in enumerate(bank_schedule(rng)):
        lst = []
        for key, delay, gains, chan in entries:
            d = fixed.setdefault(key, rng.normal(size=3)) if cb < 2 else rng.normal(size=3)
            lst.append((key, delay, gains, float(chan[0]), np.asarray(d, np.float32)))
        script.append((lst, counts))
    return script


# (bands, frame, taps, order, V): every value the rule names at least once.  F = 16 and 48: one partial tile; 256: exactly one;
# 300: a full tile and a partial one; 1024: four.  V = 1 drops the second entry, V = 3 the fourth (bank_schedule's own counts),
# V = 5 and 32 drop nothing.  C = 9 with the frame that is no multiple of the tile.
SHAPES = [(1, 16, 1, 0, 1), (3, 48, 15, 1, 5), (8, 300, 15, 2, 3), (8, 256, 255, 3, 5), (3, 1024, 255, 1, 32), (1, 300, 255, 3, 32),
          (8, 16, 15, 2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("bands,frame,taps,order,V", SHAPES)
def test_bit_equal_to_the_restatement(pkg, bands, frame, taps, order, V):
    ctx = ctx_for(pkg, bands)
    rng = np.random.default_rng(1000 * bands + frame + taps + 7 * order + V)
    src = ctx.create_source()
    ctx.ambisonic_render_init(src, frame, taps, V, 0.02, order)
    m = Model(table_of(pkg, ctx, taps), frame, V, order)
    heard = dropped = 0
    for _ in range(-(-160 // frame)):   # the script's delays reach 140 samples: a history that long first, so that every callback is heard
        blk = noise(rng, 1, frame)[0]
        assert_same(one(ctx, src, blk, []), m.process(blk, []), "priming")
    for cb, (entries, counts) in enumerate(ambisonic_schedule(rng)):
        blk = noise(rng, 1, frame)[0]   # (L != R)
        want = m.process(blk, entries)
        if V == 3:
            assert want[1] == counts, f"callback {cb + 1}: the yardstick's own counts"
        got = one(ctx, src, blk, entries)
        assert got[0].shape == (frame, channels(order))
        assert_same(got, want, f"callback {cb + 1}")
        heard += bool(got[0].any())
        dropped += got[1][3]
        if cb == 7:
            assert not got[0].any(), "a row without a sounding slot is exactly zero"
    assert heard >= 6 and (dropped > 0) == (V <= 3)
    ctx.destroy_source(src)


def mono(rng, frame):
    return np.repeat(rng.uniform(-1.0, 1.0, frame).astype(np.float32), 2)


@pytest.mark.gpu
def test_order_0_is_channel_0_of_the_reflection_renderer(pkg):
    """the yardstick this code did not write.  A mono source in both channels, order 0 (Y_0 = 1: w = gain): the one channel equals
    the left channel of fs_reflection_render_process_batch with channel_gain = (gain, gain), to the bit, over the eight-callback
    script"""
    for bands, frame, taps in ((3, 64, 15), (8, 300, 255)):
        ctx = ctx_for(pkg, bands)
        a, b = ctx.create_source(), ctx.create_source()
        ctx.ambisonic_render_init(a, frame, taps, 3, 0.02, 0)
        ctx.reflection_render_init(b, frame, taps, 3, 0.02)
        rng = np.random.default_rng(frame + taps)
        heard = False
        for cb, (entries, counts) in enumerate(ambisonic_schedule(rng)):
            blk = mono(rng, frame)
            got = one(ctx, a, blk, entries)
            want, wrow = ctx.reflection_render_process_batch([b], blk[None], [[(key, delay, gains, (g, g)) for key, delay, gains, g, _ in entries]])
            assert got[1] == counts == tuple(int(x) for x in wrow[0])
            assert got[0].shape == (frame, 1)
            assert got[0][:, 0].tobytes() == want[0][0::2].tobytes(), f"bands {bands}, F {frame}, T {taps}, callback {cb + 1}"
            assert want[0][0::2].tobytes() == want[0][1::2].tobytes()
            heard = heard or bool(got[0].any())
        assert heard
        ctx.destroy_source(a)
        ctx.destroy_source(b)


@pytest.mark.gpu
def test_every_channel_pair_is_the_reflection_renderer(pkg):
    """order 3: channels (2 k, 2 k + 1), k = 0 .. 7, equal the two channels of fs_reflection_render_process_batch fed
    channel_gain = (g Y_2k, g Y_2k+1) with Y from fs_ambisonic_encode and the product in fp32 — eight reflection sources beside the
    ambisonic one, the same mono input, over the eight-callback script: every channel of the bus, to the bit"""
    ctx = ctx_for(pkg, 3)
    frame, taps = 300, 15
    rng = np.random.default_rng(33)
    a = ctx.create_source()
    ctx.ambisonic_render_init(a, frame, taps, 3, 0.02, 3)
    refs = [ctx.create_source() for _ in range(8)]
    for s in refs:
        ctx.reflection_render_init(s, frame, taps, 3, 0.02)
    for cb, (entries, counts) in enumerate(ambisonic_schedule(rng)):
        blk = mono(rng, frame)
        got = one(ctx, a, blk, entries)
        assert got[1] == counts
        w = [F32(g) * pkg.Context.ambisonic_encode(3, d) for _, _, _, g, d in entries]
        assert all(x.dtype == np.float32 for x in w)
        lists = [[(key, delay, gains, (w[e][2 * k], w[e][2 * k + 1])) for e, (key, delay, gains, _, _) in enumerate(entries)] for k in range(8)]
        want, wrows = ctx.reflection_render_process_batch(refs, np.stack([blk] * 8), lists)
        for k in range(8):
            assert tuple(int(x) for x in wrows[k]) == counts
            assert got[0][:, 2 * k].tobytes() == want[k][0::2].tobytes(), f"callback {cb + 1}, channel {2 * k}"
            assert got[0][:, 2 * k + 1].tobytes() == want[k][1::2].tobytes(), f"callback {cb + 1}, channel {2 * k + 1}"
    for s in refs + [a]:
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_stereo_input_is_its_downmix(pkg):
    """a block with L != R gives what its downmix 0.5f * (L + R), given in both channels, gives — outputs and, over four
    callbacks, the histories"""
    ctx = ctx_for(pkg, 3)
    frame, taps = 300, 15
    rng = np.random.default_rng(34)
    a, b = ctx.create_source(), ctx.create_source()
    for s in (a, b):
        ctx.ambisonic_render_init(s, frame, taps, 4, 0.02, 2)
    for cb in range(4):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(k, rng.uniform(0, 900), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(3)]
        both = np.repeat(downmix(blk), 2)
        assert (blk[0::2] != blk[1::2]).any()
        assert_same(one(ctx, a, blk, entries), one(ctx, b, both, entries), f"callback {cb + 1}")
    ctx.destroy_source(a)
    ctx.destroy_source(b)


@pytest.mark.gpu
def test_full_bank(pkg):
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(32)
    frame, taps = 64, 15
    src = ctx.create_source()
    ctx.ambisonic_render_init(src, frame, taps, MAX_VOICES, 0.02, 3)
    m = Model(table_of(pkg, ctx, taps), frame, MAX_VOICES, 3)
    for cb in range(3):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(1000 + k, rng.uniform(0, 900), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(MAX_VOICES)]
        got = one(ctx, src, blk, entries)
        assert got[1] == (32, 32 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_ring_wrap(pkg):
    """max delay 400 samples, T = 15, F = 300: the ring is 1024 floats, and twenty callbacks write 6000"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(1024)
    frame, taps = 300, 15
    src = ctx.create_source()
    ctx.ambisonic_render_init(src, frame, taps, 3, 400.0 / FS, 1)
    m = Model(table_of(pkg, ctx, taps), frame, 3, 1)
    for cb in range(20):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(k, x, rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k, x in ((1, 400.0), (2, rng.uniform(0, 400)))]
        if cb % 5 == 4:
            entries = entries[:1]   # the second voice ends, and starts again in the next callback
        assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


@pytest.mark.gpu
def test_longest_filter(pkg):
    """T = FS_DIRECT_RENDER_MAX_TAPS = 2047 at F = 16, order 3"""
    ctx = ctx_for(pkg, 8)
    src = ctx.create_source()
    rng = np.random.default_rng(2047)
    frame, taps = 16, 2047
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    ctx.ambisonic_render_init(src, frame, taps, 2, 0.02, 3)
    m = Model(table_of(pkg, ctx, taps), frame, 2, 3)
    for cb, (da, db) in enumerate(((300.5, 10.0), (303.25, 4.75), (303.25, 4.75))):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(1, da, g[0], 0.9, rng.normal(size=3)), entry(2, db, g[1], -0.3, rng.normal(size=3))]
        assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"callback {cb + 1}")
    ctx.destroy_source(src)


# ---- physics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_left_and_right_on_the_y_channel(pkg):
    """one voice from the left (-y in the head frame) gives a Y channel (ACN 1) with W's values — the sign of W — and one from the
    right W's values negated; Z and X stay exactly zero.  By value: Y_1 is exactly +1 and -1 there"""
    ctx = ctx_for(pkg, 3)
    frame, taps = 64, 15
    rng = np.random.default_rng(35)
    g = rng.uniform(0.2, 1.0, 8).astype(np.float32)
    for direction, sign in (((0.0, -2.0, 0.0), 1.0), ((0.0, 0.5, 0.0), -1.0)):
        src = ctx.create_source()
        ctx.ambisonic_render_init(src, frame, taps, 2, 0.02, 1)
        for cb in range(2):
            out, row = one(ctx, src, mono(rng, frame), [entry(1, 30.5, g, 0.8, direction)])
        assert row == (1, 0, 0, 0) and out[:, 0].any()
        assert np.array_equal(out[:, 1], F32(sign) * out[:, 0])
        assert not out[:, 2].any() and not out[:, 3].any()
        ctx.destroy_source(src)


@pytest.mark.gpu
def test_projection_decoder_points_at_the_voice(pkg):
    """an order-3 run of one voice at azimuth 100 degrees towards the right, on the horizon, decoded by plain projection —
    speaker k's signal is sum_c Y_c(p_k) out(s, c) — onto 12 horizontal directions 30 degrees apart: the most energy is on the
    direction nearest the voice, 90 degrees.  In exact arithmetic speaker k carries y (P_0 + P_1 + P_2 + P_3)(cos gamma_k), gamma_k
    the angle to the voice, and the sum of Legendre polynomials is largest at gamma = 0"""
    ctx = ctx_for(pkg, 3)
    frame, taps = 256, 15
    rng = np.random.default_rng(36)
    src = ctx.create_source()
    ctx.ambisonic_render_init(src, frame, taps, 2, 0.02, 3)
    az = np.deg2rad(100.0)
    voice = (np.cos(az), np.sin(az), 0.0)
    g = rng.uniform(0.2, 1.0, 8).astype(np.float32)
    for cb in range(2):
        out, row = one(ctx, src, mono(rng, frame), [entry(1, 30.5, g, 1.0, voice)])
    speakers = [(np.cos(np.deg2rad(30.0 * k)), np.sin(np.deg2rad(30.0 * k)), 0.0) for k in range(12)]
    decode = np.stack([pkg.Context.ambisonic_encode(3, p) for p in speakers]).astype(np.float64)   # [12][16]
    energy = ((out.astype(np.float64) @ decode.T) ** 2).sum(axis=0)
    print("projection decoder, energy per speaker relative to the loudest:", np.round(energy / energy.max(), 3))
    assert int(np.argmax(energy)) == 3 and energy[3] > 0.0
    ctx.destroy_source(src)


# ---- contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_single_and_permuted_agree(pkg):
    """sources of 1, 3 and 8 slots with 0, 1 and 5 entries (rotating) in one batch of stride 5, order 2; the mix with out, and
    alone"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(3)
    frame, taps, n, order = 300, 15, 3, 2
    V = [1, 3, 8]
    sets = [[ctx.create_source() for _ in range(n)] for _ in range(3)]   # one call | three calls | permuted order
    for group in sets:
        for s, v in zip(group, V):
            ctx.ambisonic_render_init(s, frame, taps, v, 0.02, order)
    models = [Model(table_of(pkg, ctx, taps), frame, v, order) for v in V]
    perm = [2, 0, 1]
    counts = [[0, 1, 5], [1, 5, 0], [5, 0, 1], [1, 1, 5]]
    for cb in range(4):
        blk = noise(rng, n, frame)
        lists = [[entry(50 + k, rng.uniform(0, 600), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(counts[cb][i])]
                 for i in range(n)]
        out, mix, rows = ctx.ambisonic_render_process_batch(sets[0], blk, lists, stride=5, want_mix=True)
        singles = [one(ctx, sets[1][i], blk[i], lists[i], stride=5) for i in range(n)]
        pout, pmix, prows = ctx.ambisonic_render_process_batch([sets[2][i] for i in perm], blk[perm], [lists[i] for i in perm], stride=5,
                                                               want_mix=True)
        for i in range(n):
            want = models[i].process(blk[i], lists[i])
            assert_same((out[i], tuple(int(x) for x in rows[i])), want, f"batch {cb} {i}")
            assert_same(singles[i], want, f"single {cb} {i}")
            j = perm.index(i)
            assert_same((pout[j], tuple(int(x) for x in prows[j])), want, f"permuted {cb} {i}")
        assert mix.shape == (frame, channels(order))
        assert mix.tobytes() == mix_model(out).tobytes(), "mix is not the fp32 sum in list order"
        assert pmix.tobytes() == mix_model(pout).tobytes()
    blk2 = noise(rng, n, frame)   # with out == NULL only the mix comes back; the state moves on all the same
    only_mix, rows2 = ctx.ambisonic_render_process_batch(sets[0], blk2, lists, stride=5, want_out=False, want_mix=True)
    wants = [models[i].process(blk2[i], lists[i]) for i in range(n)]
    assert only_mix.shape == (frame, channels(order)) and only_mix.tobytes() == mix_model([w[0] for w in wants]).tobytes()
    assert [tuple(int(x) for x in r) for r in rows2] == [w[1] for w in wants]
    blk3 = noise(rng, n, frame)   # ... and out alone
    only_out, rows3 = ctx.ambisonic_render_process_batch(sets[0], blk3, lists, stride=5)
    for i in range(n):
        assert_same((only_out[i], tuple(int(x) for x in rows3[i])), models[i].process(blk3[i], lists[i]), f"out only {i}")
    for s in sum(sets, []):
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    """two contexts fed the same good callbacks; one of them also sees every refusal.  After the refusals a callback's output on the
    two is the same, and the yardstick's"""
    cap = pkg._capi
    lib = cap.load()
    ctx, twin = pkg.Context(num_bands=3), pkg.Context(num_bands=3)
    rng = np.random.default_rng(5)
    frame, taps, order = 64, 15, 2
    Cn = channels(order)
    srcs, twins = [ctx.create_source() for _ in range(3)], [twin.create_source() for _ in range(3)]
    for group, c in ((srcs, ctx), (twins, twin)):
        for s, v in zip(group, (2, 3, 4)):
            c.ambisonic_render_init(s, frame, taps, v, 0.01, order)   # D = 480
    other_frame, other_taps, other_order, uninit, dead = (ctx.create_source() for _ in range(5))
    ctx.ambisonic_render_init(other_frame, 128, taps, 3, 0.01, order)
    ctx.ambisonic_render_init(other_taps, frame, 31, 3, 0.01, order)
    ctx.ambisonic_render_init(other_order, frame, taps, 3, 0.01, order + 1)
    ctx.ambisonic_render_init(dead, frame, taps, 3, 0.01, order)
    ctx.reflection_render_init(uninit, frame, taps, 3, 0.01)   # (another renderer's state is not this one's)
    ctx.destroy_source(dead)
    models = [Model(table_of(pkg, ctx, taps), frame, v, order) for v in (2, 3, 4)]
    gains = np.full(8, 0.5, np.float32)

    def good_call():
        blk = noise(rng, 3, frame)
        lists = [[entry(k, rng.uniform(0, 400), gains, 0.5, rng.normal(size=3)) for k in range(2)] for _ in range(3)]
        out, rows = ctx.ambisonic_render_process_batch(srcs, blk, lists)
        tout, trows = twin.ambisonic_render_process_batch(twins, blk, lists)
        assert out.tobytes() == tout.tobytes() and rows.tobytes() == trows.tobytes(), "the context that saw the refusals differs"
        for i in range(3):
            assert_same((out[i], tuple(int(x) for x in rows[i])), models[i].process(blk[i], lists[i]), f"source {i}")

    good_call()
    blk = noise(rng, 3, frame)
    sentinel = np.full((3, frame, Cn + 7), 7.0, np.float32)   # (room for a row of the higher order)
    out, mix = sentinel.copy(), sentinel[0].copy()
    rows = np.full((3, 4), 7, np.uint32)
    inf, nan = float("inf"), float("nan")
    base = np.zeros((3, 2), dtype=pkg.Context.AMBISONIC_VOICE_DTYPE)
    for i in range(3):
        for e in range(2):
            base[i, e] = (e, 0.001 * (i + e + 1), gains, 0.5, (0.0, 1.0, 0.5))

    def call(sources=srcs, count=3, table=base, counts=(2, 2, 2), stride=2, blocks=blk, dest=out, mixed=None, voices=True, cnts=True, handles=True):
        arr = (C.c_int32 * len(sources))(*sources)
        t = np.ascontiguousarray(table)
        n = np.asarray(counts, np.int32)
        return lib.fs_ambisonic_render_process_batch(ctx.h, arr if handles else None, count, blocks.ctypes.data if blocks is not None else None,
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
    wide = np.zeros((3, 33), dtype=pkg.Context.AMBISONIC_VOICE_DTYPE)
    for stride, table in ((0, base), (-1, base), (33, wide)):
        assert call(stride=stride, table=table, counts=(0, 0, 0)) == cap.ERR_INVALID_ARGUMENT, stride
    assert call(table=with_entry("key", 0)) == cap.ERR_INVALID_ARGUMENT, "a key twice in one row"
    for v in (-0.001, nan, inf, 481.0 / FS):
        assert call(table=with_entry("delay", v)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (-0.5, nan, inf):
        assert call(table=with_entry("band_gain", v, 1)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (nan, inf, -inf):
        assert call(table=with_entry("gain", v)) == cap.ERR_INVALID_ARGUMENT, v
    for v in (nan, inf, -inf):   # a component that is not finite
        for axis in range(3):
            assert call(table=with_entry("direction", v, axis)) == cap.ERR_INVALID_ARGUMENT, (v, axis)
    for d in ((0.0, -0.0, 0.0), (1e-16, 0.0, 0.0), (1e-20, 1e-20, 1e-20), (2e15, 0.0, 0.0), (3e19, 3e19, 0.0)):   # the zero vector, a squared length out of range
        assert call(table=with_entry("direction", d)) == cap.ERR_INVALID_ARGUMENT, d
    for count in (0, -1, 257):
        assert call(count=count) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], srcs[1], srcs[0]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_frame, srcs[2]]) == cap.ERR_INVALID_ARGUMENT
    assert call(sources=[srcs[0], other_taps, srcs[2]]) == cap.ERR_INVALID_ARGUMENT, "sources whose T differ"
    assert call(sources=[srcs[0], other_order, srcs[2]]) == cap.ERR_INVALID_ARGUMENT, "mixed orders in one call"
    assert call(sources=[other_order, srcs[1], srcs[2]]) == cap.ERR_INVALID_ARGUMENT, "mixed orders in one call, the higher first"
    assert call(sources=[srcs[0], uninit, srcs[2]]) == cap.ERR_INVALID_ARGUMENT, "a source without init"
    assert call(sources=[srcs[0], dead, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[srcs[0], 12345, srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(sources=[-1, srcs[1], srcs[2]]) == cap.ERR_BAD_HANDLE
    assert call(handles=False) == cap.ERR_INVALID_ARGUMENT
    assert call(blocks=None) == cap.ERR_INVALID_ARGUMENT
    assert call(voices=False) == cap.ERR_INVALID_ARGUMENT
    assert call(cnts=False) == cap.ERR_INVALID_ARGUMENT
    assert call(dest=None) == cap.ERR_INVALID_ARGUMENT, "out == NULL && mix == NULL"
    assert call(table=with_entry("direction", nan, 0), mixed=mix) == cap.ERR_INVALID_ARGUMENT
    assert np.array_equal(out, sentinel) and np.array_equal(mix, sentinel[0]) and np.all(rows == 7), "a refused call wrote"
    good_call()   # every refused call left all three sources as they were

    # init refusals; a refused init leaves the source as it was
    for args in ((15, 15, 3, 0.01, 2), (16385, 15, 3, 0.01, 2), (frame, 16, 3, 0.01, 2), (frame, 0, 3, 0.01, 2), (frame, 2049, 3, 0.01, 2),
                 (frame, taps, 0, 0.01, 2), (frame, taps, -1, 0.01, 2), (frame, taps, 33, 0.01, 2), (frame, taps, 3, -0.01, 2),
                 (frame, taps, 3, nan, 2), (frame, taps, 3, inf, 2), (frame, taps, 3, 22.0, 2),
                 (frame, taps, 2, 0.01, -1), (frame, taps, 2, 0.01, 4), (frame, taps, 2, 0.01, 16)):
        assert lib.fs_ambisonic_render_init(ctx.h, srcs[0], args[0], args[1], args[2], C.c_float(args[3]), args[4]) == cap.ERR_INVALID_ARGUMENT, args
    assert lib.fs_ambisonic_render_init(ctx.h, 12345, frame, taps, 3, C.c_float(0.01), 1) == cap.ERR_BAD_HANDLE
    assert lib.fs_ambisonic_render_release(ctx.h, 12345) == cap.ERR_BAD_HANDLE
    assert lib.fs_ambisonic_render_release(ctx.h, uninit) == cap.OK
    good_call()
    blk = noise(rng, 3, frame)
    got = np.zeros((3, frame, Cn), np.float32)
    assert call(table=with_entry("band_gain", nan, 3), blocks=blk, dest=got) == cap.OK, "entries beyond num_bands are ignored"
    for i in range(3):   # (that call was a callback like any other)
        lst = [(int(base[i, e]["key"]), float(base[i, e]["delay"]), gains, 0.5, (0.0, 1.0, 0.5)) for e in range(2)]
        assert_same((got[i], tuple(int(x) for x in rows[i])), models[i].process(blk[i], lst), f"source {i}")
    ctx.close()
    twin.close()


@pytest.mark.gpu
def test_release_and_reinit_with_another_order(pkg):
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(8)
    src = ctx.create_source()
    frame, taps, V = 64, 15, 3
    ctx.ambisonic_render_init(src, frame, taps, V, 0.02, 1)
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    entries = [entry(1, 50.5, g[0], 1.0, (0.0, 1.0, 0.2)), entry(2, 300.0, g[1], -0.5, (1.0, -1.0, 0.0))]
    for _ in range(2):
        one(ctx, src, noise(rng, 1, frame)[0], entries)
    ctx.ambisonic_render_release(src)   # zero history, every slot free: the same keys fade in from silence
    m = Model(table_of(pkg, ctx, taps), frame, V, 1)
    for cb in range(2):
        blk = noise(rng, 1, frame)[0]
        got = one(ctx, src, blk, entries)
        assert got[1] == (2, 2 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"after release, callback {cb + 1}")
    for frame, taps, V, order in ((300, 15, 1, 3), (64, 255, 5, 0), (64, 15, 3, 2)):   # another order, F, T and V — with voices held
        ctx.ambisonic_render_init(src, frame, taps, V, 0.02, order)
        m = Model(table_of(pkg, ctx, taps), frame, V, order)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            got = one(ctx, src, blk, entries)
            assert got[0].shape == (frame, channels(order))
            assert_same(got, m.process(blk, entries), f"{(frame, taps, V, order)} callback {cb + 1}")
    ctx.destroy_source(src)   # with voices held
    closing = pkg.Context(num_bands=1)   # fs_context_destroy with a source and held voices
    s = closing.create_source()
    closing.ambisonic_render_init(s, 64, 15, 2, 0.02, 3)
    one(closing, s, noise(rng, 1, 64)[0], entries)
    closing.close()


@pytest.mark.gpu
def test_steady_state_allocates_nothing(pkg):
    ctx = pkg.Context(num_bands=3)
    rng = np.random.default_rng(40)
    frame, taps, n = 64, 15, 40
    srcs = [ctx.create_source() for _ in range(n)]
    for s in srcs:
        ctx.ambisonic_render_init(s, frame, taps, 4, 0.01, 3)
    blk = noise(rng, n, frame)
    lists = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.0)) for k in range(3)]] * n
    ctx.ambisonic_render_process_batch(srcs, blk, lists[:n], stride=4, want_mix=True)
    free0 = device_free_bytes()
    for cb in range(20):
        more = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.1 * cb)) for k in range(cb % 2, 4)]] * n   # slots fill up and turn over
        ctx.ambisonic_render_process_batch(srcs, blk, more, stride=4, want_mix=True)
    ctx.ambisonic_render_process_batch(srcs[:7], blk[:7], lists[:7], stride=3)   # a smaller shape fits what is there
    assert device_free_bytes() >= free0
    ctx.close()


@pytest.mark.gpu
def test_staging_is_its_own(pkg):
    """one "audio callback" = a direct batch of 5, a reflection batch of 3, a binaural batch of 4 and an ambisonic batch of 2, three
    rounds; the ambisonic rows equal what they give alone, and so do the others beside them"""
    frame, taps = 64, 15
    rng = np.random.default_rng(77)
    the_set = (AXES.copy(), rng.uniform(-1.0, 1.0, (6, 2, 7)).astype(np.float32))
    dir_blocks = [noise(rng, 5, frame) for _ in range(3)]
    ref_blocks = [noise(rng, 3, frame) for _ in range(3)]
    bin_blocks = [noise(rng, 4, frame) for _ in range(3)]
    amb_blocks = [noise(rng, 2, frame) for _ in range(3)]
    tg = [[(float(F32(rng.uniform(0, 400) / FS)), rng.uniform(0, 1, 8).astype(np.float32)) for _ in range(5)] for _ in range(3)]
    ref_lists = [[[(k, secs(rng.uniform(0, 400)), rng.uniform(0, 1, 8).astype(np.float32), rng.uniform(-1, 1, 2).astype(np.float32))
                   for k in range(2 + cb)] for _ in range(3)] for cb in range(3)]
    dir_lists = [[[entry(k, rng.uniform(0, 400), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(1 + cb)]
                  for _ in range(4)] for cb in range(3)]

    def run(direct, reflect, binaural, ambisonic):
        ctx = pkg.Context(num_bands=1)
        ctx.hrtf_set(*the_set)
        ds = [ctx.create_source() for _ in range(5)]
        es = [ctx.create_source() for _ in range(3)]
        bs = [ctx.create_source() for _ in range(4)]
        ms = [ctx.create_source() for _ in range(2)]
        for s in ds:
            ctx.direct_render_init(s, frame, taps, 0.01)
        for s in es:
            ctx.reflection_render_init(s, frame, taps, 4, 0.01)
        for s in bs:
            ctx.binaural_render_init(s, frame, taps, 4, 0.01)
        for s in ms:
            ctx.ambisonic_render_init(s, frame, taps, 4, 0.01, 3)
        outs = {"direct": [], "reflect": [], "binaural": [], "ambisonic": []}
        for cb in range(3):
            if direct:
                outs["direct"].append(ctx.direct_render_process_batch(ds, dir_blocks[cb], tg[cb]).tobytes())
            if reflect:
                out, rows = ctx.reflection_render_process_batch(es, ref_blocks[cb], ref_lists[cb])
                outs["reflect"].append(out.tobytes() + rows.tobytes())
            if binaural:
                out, rows = ctx.binaural_render_process_batch(bs, bin_blocks[cb], dir_lists[cb])
                outs["binaural"].append(out.tobytes() + rows.tobytes())
            if ambisonic:
                out, mix, rows = ctx.ambisonic_render_process_batch(ms, amb_blocks[cb], dir_lists[cb][:2], want_mix=True)
                outs["ambisonic"].append(out.tobytes() + mix.tobytes() + rows.tobytes())
        ctx.close()
        return outs

    together = run(True, True, True, True)
    assert together["ambisonic"] == run(False, False, False, True)["ambisonic"], "the ambisonic rows changed beside the other batches"
    assert together["direct"] == run(True, False, False, False)["direct"], "the direct rows changed beside the other batches"
    assert together["reflect"] == run(False, True, False, False)["reflect"], "the reflection rows changed beside the other batches"
    assert together["binaural"] == run(False, False, True, False)["binaural"], "the binaural rows changed beside the other batches"


@pytest.mark.gpu
def test_one_source_holds_four_renderers(pkg):
    """direct, reflection, binaural and ambisonic state side by side on ONE source: the ambisonic output is what a source of its own
    gives, and the reflection renderer's beside it likewise"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(12)
    frame, taps = 64, 15
    ctx.hrtf_set(AXES.copy(), rng.uniform(-1.0, 1.0, (6, 2, 7)).astype(np.float32))
    both, alone, ref_alone = ctx.create_source(), ctx.create_source(), ctx.create_source()
    ctx.direct_render_init(both, frame, taps, 0.02)
    ctx.reflection_render_init(both, frame, taps, 2, 0.02)
    ctx.binaural_render_init(both, frame, taps, 2, 0.02)
    ctx.ambisonic_render_init(both, frame, taps, 2, 0.02, 2)
    ctx.ambisonic_render_init(alone, frame, taps, 2, 0.02, 2)
    ctx.reflection_render_init(ref_alone, frame, taps, 2, 0.02)
    g = rng.uniform(0, 1, 8).astype(np.float32)
    for cb in range(3):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(1, 90.0 + 7.3 * cb, g, 0.8, rng.normal(size=3))]
        ctx.direct_render_process_batch([both], blk[None], [(secs(50.0), g)])
        ref = [[(3, secs(70.0), g, (0.5, 0.5))]]
        got_ref = ctx.reflection_render_process_batch([both], blk[None], ref)
        ctx.binaural_render_process_batch([both], blk[None], [entries])
        assert_same(one(ctx, both, blk, entries), one(ctx, alone, blk, entries), f"callback {cb + 1}")
        want_ref = ctx.reflection_render_process_batch([ref_alone], blk[None], ref)
        assert got_ref[0].tobytes() == want_ref[0].tobytes(), f"callback {cb + 1}: the reflection renderer beside the others"
    for s in (both, alone, ref_alone):
        ctx.destroy_source(s)


@pytest.mark.gpu
def test_component_layer(pkg):
    """UpdateDirectPaths + UpdateReflectionPaths -> FrequenSeeAudioAmbisonicPlugin.ProcessAudio in the 12-triangle shoebox, the
    listener facing +x with the right ear to +y, the source moving past 100 cm to its right: the plugin's call equals
    Context.ambisonic_render_process_batch on the entries Voices() — the binaural plugin's, inherited — returns; and while the
    source is on the right the direct voice alone has a Y channel of the opposite sign to W (AmbiX's y points left)"""
    w = shoebox_world()
    frame, taps, order = 256, 15, 2

    def world():
        sub = pkg.AudioRayTracingSubsystem(num_bands=4)
        sub.RegisterGeometry(w.tri, w.mat, object_ids=w.obj)
        sub.SetMaterials(w.absorption, w.transmission, w.scattering)
        comp = pkg.FrequenSeeAudioComponent(SRC)
        comp.OnRegister(sub)
        sub.SetListenerLocation(LIS)
        return sub, comp

    fwd, right = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    sub, comp = world()
    plug = pkg.FrequenSeeAudioAmbisonicPlugin(sub)
    plug.Initialize(frame, taps, 16, 0.05)
    plug.Order = order
    plug.OnInitSource(comp)   # (no HRIR set is needed)
    sub2, comp2 = world()
    sub2.ctx.ambisonic_render_init(comp2._src, frame, taps, 16, 0.05, order)
    sub3, comp3 = world()   # the direct voice alone
    sub3.ctx.ambisonic_render_init(comp3._src, frame, taps, 2, 0.05, 1)
    empty_row = np.zeros(1, dtype=pkg.Context.REFLECTION_ROW_DTYPE)[0]
    rng = np.random.default_rng(2)
    lis = np.asarray(LIS, np.float64)
    for cb, dx in enumerate((-60.0, -20.0, 20.0, 60.0)):   # past the listener, 100 cm to its right
        pos = [float(lis[0] + dx), float(lis[1] + 100.0), float(lis[2])]
        comp.SetComponentLocation(pos)
        direct = sub.UpdateDirectPaths()
        rows, paths = sub.UpdateReflectionPaths(max_paths=8)
        blk = mono(rng, frame)[None]
        got, gmix, grow = plug.ProcessAudio([comp], blk, rows, paths, fwd, right, reference_length=500.0, direct=(direct, LIS), want_mix=True)
        voices = plug.Voices(rows[0], paths[0], fwd, right, 500.0, direct=(direct[0], np.asarray(pos) - lis))
        assert voices.dtype == pkg.Context.AMBISONIC_VOICE_DTYPE and voices.shape == (1 + int(rows[0]["returned"]),)
        assert voices["direction"][0][1] > 0.0, "the source is on the right"
        want, wrow = sub2.ctx.ambisonic_render_process_batch([comp2._src], blk, [voices])
        assert int(grow[0]["dropped"]) == 0 and int(grow[0]["sounding"]) == voices.shape[0]
        assert got.shape == (1, frame, channels(order)) and got.any()
        assert got.tobytes() == want.tobytes() and grow.tobytes() == wrow.tobytes()
        assert gmix.tobytes() == got[0].tobytes(), "the mix of one row is the row"
        only = plug.Voices(empty_row, paths[0], fwd, right, 500.0, direct=(direct[0], np.asarray(pos) - lis))
        heard = sub3.ctx.ambisonic_render_process_batch([comp3._src], blk, [only])[0][0]
        loud = np.abs(heard[:, 0]) > 1e-3
        assert loud.any() and np.all(np.sign(heard[loud, 1]) == -np.sign(heard[loud, 0]))
    plug.OnReleaseSource(comp)
    for s in (sub, sub2, sub3):
        s.Deinitialize()
