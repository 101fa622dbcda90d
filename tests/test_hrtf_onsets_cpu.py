"""Onset-aligned HRIRs, the part that needs no device (include/frequensee.h, "Onsets"): fs_hrtf_delay and fs_hrtf_split_onsets
against their numpy float32 restatements, bit for bit, with their refusals and their round trip; fs_hrtf_spherical_head_split
against a float64 restatement and, delayed, against fs_hrtf_spherical_head under a derived bound; the exports; and
FrequenSeeAudioBinauralPlugin.SetHrtf(align=True) on a context that records the library calls."""
import types

import numpy as np
import pytest

from hrtf_onsets_model import delay32, split32

F32 = np.float32
FS = 48000
U = 2.0 ** -24
NEW = ("fs_hrtf_set_onsets", "fs_hrtf_onsets_info", "fs_hrtf_delay", "fs_hrtf_split_onsets", "fs_hrtf_spherical_head_split")


def test_exports(pkg):
    lib = pkg._capi.load()
    for name in NEW:
        assert name in pkg._capi.EXPORTS and hasattr(lib, name)
    assert lib.fs_abi_version() == 5
    for name in ("hrtf_set_onsets", "hrtf_onsets_info", "hrtf_delay", "hrtf_split_onsets", "hrtf_spherical_head_split"):
        assert hasattr(pkg.Context, name)


# ---- fs_hrtf_delay -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 2, 7, 128])
def test_delay_is_the_restatement(pkg, H):
    rng = np.random.default_rng(H)
    for tau in (0.0, 0.5, 3.0, 6.5, 31.999998):
        h = rng.uniform(-1.0, 1.0, H).astype(np.float32)
        h[rng.integers(0, H)] = 0.0
        least = H + int(F32(tau)) + 1
        for taps in (least, least + 5):
            got = pkg.Context.hrtf_delay(h, tau, taps)
            assert got.tobytes() == delay32(h, tau, taps).tobytes(), (H, tau, taps)
        assert pkg.Context.hrtf_delay(h, tau).shape == (least,)
    # known answers: an integer delay moves the taps, half a sample halves two neighbours
    h = np.arange(1, H + 1, dtype=np.float32)
    assert np.array_equal(pkg.Context.hrtf_delay(h, 3.0), np.concatenate([np.zeros(3, np.float32), h, np.zeros(1, np.float32)]))
    half = pkg.Context.hrtf_delay(np.ones(1, np.float32), 6.5)
    assert half.tolist() == [0.0] * 6 + [0.5, 0.5]
    assert F32(31.999998) < 32 and int(F32(31.999998)) == 31


def test_delay_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    h, out = np.ones(7, np.float32), np.full(64, 7.0, np.float32)
    nan, inf = float("nan"), float("inf")
    bad = [("NULL h", (None, 7, 1.0, out.ctypes.data, 64)), ("NULL out", (h.ctypes.data, 7, 1.0, None, 64)), ("H = 0", (h.ctypes.data, 0, 1.0, out.ctypes.data, 64)),
           ("H < 0", (h.ctypes.data, -1, 1.0, out.ctypes.data, 64)), ("tau < 0", (h.ctypes.data, 7, -0.5, out.ctypes.data, 64)),
           ("tau nan", (h.ctypes.data, 7, nan, out.ctypes.data, 64)), ("tau inf", (h.ctypes.data, 7, inf, out.ctypes.data, 64)),
           ("tau huge", (h.ctypes.data, 7, 3e9, out.ctypes.data, 64)), ("He one short", (h.ctypes.data, 7, 6.5, out.ctypes.data, 13)),
           ("He = 0", (h.ctypes.data, 7, 0.0, out.ctypes.data, 0)), ("He < 0", (h.ctypes.data, 7, 0.0, out.ctypes.data, -3))]
    for what, args in bad:
        assert lib.fs_hrtf_delay(*args) == cap.ERR_INVALID_ARGUMENT, what
        assert np.all(out == 7.0), f"{what}: a refused call wrote"
    assert lib.fs_hrtf_delay(h.ctypes.data, 7, 6.5, out.ctypes.data, 14) == cap.OK and np.all(out[:14] != 7.0) and np.all(out[14:] == 7.0)
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.hrtf_delay(h, -1.0)
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.hrtf_delay(h, 2.0, 9)


# ---- fs_hrtf_split_onsets ------------------------------------------------------------------------------------------------------
def planted(rng, n, H):
    """random HRIRs with an onset planted per (direction, ear): small taps (below a tenth of the peak) before it, one of them
    exactly at the threshold's other side, an all-zero one, one whose peak is its first tap"""
    h = np.zeros((n, 2, H), np.float32)
    want = rng.integers(0, H - 4, (n, 2))
    for j in range(n):
        for ear in range(2):
            k0 = int(want[j, ear])
            h[j, ear, :k0] = rng.uniform(-0.04, 0.04, k0)
            h[j, ear, k0:] = rng.uniform(-1.0, 1.0, H - k0) * np.exp(-0.2 * np.arange(H - k0))
            h[j, ear, k0] = 0.9 * (-1) ** j
    h[1, 0] = 0.0
    want[1, 0] = 0
    h[2, 1, 0], want[2, 1] = 1.0, 0
    return h, want


def test_split_is_the_restatement(pkg):
    rng = np.random.default_rng(5)
    for n, H in ((1, 5), (6, 32), (16, 128)):
        h, want = planted(rng, max(n, 3), H) if H > 5 else (rng.uniform(-1, 1, (n, 2, H)).astype(np.float32), None)
        for threshold, lead in ((0.1, 0), (0.1, 2), (1.0, 0), (0.5, 1000), (1e-3, 1)):
            aligned, onsets = pkg.Context.hrtf_split_onsets(h, threshold, lead)
            a32, o32 = split32(h, threshold, lead)
            assert aligned.tobytes() == a32.tobytes() and onsets.tobytes() == o32.tobytes(), (n, H, threshold, lead)
            assert np.all(onsets >= 0) and np.all(onsets == np.floor(onsets))
            if lead == 1000:
                assert not onsets.any(), "lead is clipped at 0"
            if want is not None and threshold == 0.1:
                assert np.array_equal(onsets, np.maximum(want - lead, 0).astype(np.float32)), "the planted onsets"
                assert onsets[1, 0] == 0 and not aligned[1, 0].any(), "an all-zero HRIR"
            # in place
            both = h.copy()
            o2 = np.zeros_like(onsets)
            rc = pkg._capi.load().fs_hrtf_split_onsets(both.ctypes.data, h.shape[0], H, threshold, lead, both.ctypes.data, o2.ctypes.data)
            assert rc == pkg._capi.OK and both.tobytes() == aligned.tobytes() and o2.tobytes() == onsets.tobytes(), "in place"
            # the round trip, on the same HRIRs with nothing before their onsets (what the split cuts off is gone): delaying each
            # aligned HRIR by its integer onset returns the original by value
            clean = h.copy()
            for j in range(h.shape[0]):
                for ear in range(2):
                    clean[j, ear, :int(onsets[j, ear])] = 0.0
            aligned, again = pkg.Context.hrtf_split_onsets(clean, threshold, lead)
            assert again.tobytes() == onsets.tobytes()
            for j in range(h.shape[0]):
                for ear in range(2):
                    o = int(onsets[j, ear])
                    back = pkg.Context.hrtf_delay(aligned[j, ear], float(o), H + o + 1)
                    assert np.array_equal(back[:H], clean[j, ear]) and not back[H:].any(), (j, ear)


def test_split_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    h = np.ones((3, 2, 8), np.float32)
    a, o = np.full((3, 2, 8), 7.0, np.float32), np.full((3, 2), 7.0, np.float32)
    nan = float("nan")
    bad = [("NULL hrir", (None, 3, 8, 0.1, 0, a.ctypes.data, o.ctypes.data)), ("NULL aligned", (h.ctypes.data, 3, 8, 0.1, 0, None, o.ctypes.data)),
           ("NULL onsets", (h.ctypes.data, 3, 8, 0.1, 0, a.ctypes.data, None)), ("n = 0", (h.ctypes.data, 0, 8, 0.1, 0, a.ctypes.data, o.ctypes.data)),
           ("H = 0", (h.ctypes.data, 3, 0, 0.1, 0, a.ctypes.data, o.ctypes.data)), ("threshold 0", (h.ctypes.data, 3, 8, 0.0, 0, a.ctypes.data, o.ctypes.data)),
           ("threshold > 1", (h.ctypes.data, 3, 8, 1.5, 0, a.ctypes.data, o.ctypes.data)), ("threshold nan", (h.ctypes.data, 3, 8, nan, 0, a.ctypes.data, o.ctypes.data)),
           ("threshold < 0", (h.ctypes.data, 3, 8, -0.1, 0, a.ctypes.data, o.ctypes.data)), ("lead < 0", (h.ctypes.data, 3, 8, 0.1, -1, a.ctypes.data, o.ctypes.data))]
    for what, args in bad:
        assert lib.fs_hrtf_split_onsets(*args) == cap.ERR_INVALID_ARGUMENT, what
        assert np.all(a == 7.0) and np.all(o == 7.0), f"{what}: a refused call wrote"
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.hrtf_split_onsets(h, 0.0)


# ---- fs_hrtf_spherical_head_split ----------------------------------------------------------------------------------------------
def head64(fs, n, H, a=8.75, c=34300.0):
    """the header's model in float64 with its halves apart: (dirs, g [n][2][H], tau fs [n][2])"""
    a_c = float(F32(a)) / float(F32(c))
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    dirs = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
    g, onsets = np.zeros((n, 2, H)), np.zeros((n, 2))
    for ear in range(2):
        theta = np.arccos(np.clip(dirs[:, 1] * (-1.0 if ear == 0 else 1.0), -1.0, 1.0))
        tau = np.where(theta <= np.pi / 2, a_c * (1.0 - np.cos(theta)), a_c * (1.0 + theta - np.pi / 2))
        alpha = 1.05 + 0.95 * np.cos(theta * np.pi / (5.0 * np.pi / 6.0))
        kappa = fs * a_c
        b0, b1, a1 = (1.0 + alpha * kappa) / (1.0 + kappa), (1.0 - alpha * kappa) / (1.0 + kappa), (1.0 - kappa) / (1.0 + kappa)
        g[:, ear, 0] = b0
        g[:, ear, 1] = b1 - a1 * b0
        for m in range(2, H):
            g[:, ear, m] = -a1 * g[:, ear, m - 1]
        onsets[:, ear] = tau * fs
    return dirs, g, onsets


def ulp_apart(got, want64):
    """|got - want| in units of float32 ulps of want"""
    spacing = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / spacing


def test_spherical_head_split_against_float64(pkg):
    for n, H in ((6, 2), (64, 40), (1024, 96)):
        dirs, hrir, onsets = pkg.Context.hrtf_spherical_head_split(FS, n, H)
        d64, g64, o64 = head64(FS, n, H)
        assert ulp_apart(dirs, d64).max() <= 1.0 and ulp_apart(onsets, o64).max() <= 1.0
        # the filter's tail is a geometric sequence: the two libraries' cos may differ in the last place of double, which stays far
        # below one float32 ulp of each tap
        assert ulp_apart(hrir, g64).max() <= 1.0, (n, H)
        assert np.all(onsets >= 0) and onsets.max() < 8.75 / 34300.0 * (1.0 + np.pi / 2.0) * FS   # (the far side's delay: 31.5)
        same_dirs, _ = pkg.Context.hrtf_spherical_head(FS, n, 64)
        assert dirs.tobytes() == same_dirs.tobytes()


def test_delayed_split_head_is_the_head(pkg):
    """fs_hrtf_delay of the two halves against fs_hrtf_spherical_head's taps h = fl((1 - f*) g*[k - i] + f* g*[k - i - 1]), the
    starred values exact in double.  With o = fl(tau fs), |o - tau fs| <= u o, and g = fl(g*): the delayed tap is
    fl(fl(gg x_a) + fl(f x_b)) with x = fl(g*), gg = fl(1 - f).  Its distance from the exact tap is at most
      (|x_a| + |x_b|) ((1 + u)^4 - 1)        x's rounding, gg's rounding (on x_a), the product's and the sum's: at most four
                                             roundings on either term, and gg + f <= 1 + u
      + u o max_k |g*[k] - g*[k - 1]|        the onset's rounding: the tap is piecewise linear in the onset with those slopes (and
                                             continuous across an integer onset), g* = 0 before the first tap
      + u |h|                                the reference tap's own rounding to float."""
    n, H = 258, 64
    dirs, g, onsets = pkg.Context.hrtf_spherical_head_split(FS, n, H)
    _, head = pkg.Context.hrtf_spherical_head(FS, n, H)
    worst = 0.0
    for j in range(n):
        for ear in range(2):
            o = onsets[j, ear]
            hd = pkg.Context.hrtf_delay(g[j, ear], o, H + int(o) + 1)[:H].astype(np.float64)
            x = np.abs(g[j, ear].astype(np.float64))
            i = int(o)
            xa, xb = np.zeros(H + 1), np.zeros(H + 1)
            xa[i:H] = x[:H - i]
            xb[i + 1:H + 1] = x[:H - i]
            step = np.abs(np.diff(np.concatenate([[0.0], g[j, ear].astype(np.float64)]))).max()
            ref = head[j, ear].astype(np.float64)
            bound = (xa[:H] + xb[:H]) * ((1.0 + U) ** 4 - 1.0) + U * float(o) * step + U * np.abs(ref)
            err = np.abs(hd - ref)
            assert np.all(err <= bound), (j, ear, float((err / np.maximum(bound, 1e-300)).max()))
            live = bound > 0
            worst = max(worst, float((err[live] / bound[live]).max()))
    print(f"delayed split head vs the head: worst share of the bound {worst:.3f}")


def test_spherical_head_split_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    d, h, o = np.full((6, 3), 7.0, np.float32), np.full((6, 2, 8), 7.0, np.float32), np.full((6, 2), 7.0, np.float32)

    def call(fs=FS, a=8.75, c=34300.0, n=6, H=8, dp=d.ctypes.data, hp=h.ctypes.data, op=o.ctypes.data):
        return lib.fs_hrtf_spherical_head_split(fs, a, c, n, H, dp, hp, op)

    for kw in (dict(fs=0), dict(a=0.0), dict(a=float("nan")), dict(c=-1.0), dict(n=0), dict(n=4097), dict(H=1), dict(H=513), dict(dp=None),
               dict(hp=None), dict(op=None)):
        assert call(**kw) == cap.ERR_INVALID_ARGUMENT, kw
    assert np.all(d == 7.0) and np.all(h == 7.0) and np.all(o == 7.0), "a refused call wrote"
    small = np.zeros((6, 2, 2), np.float32)
    assert call(H=2, hp=small.ctypes.data) == cap.OK, "taps >= 2 suffices: the onset needs none"


# ---- the component layer's plumbing -----------------------------------------------------------------------------------------------
def test_set_hrtf_align_plumbing(pkg):
    """SetHrtf(align=True) on a context that records: the split set and its onsets for a host set, the host's own onsets where it
    has them, the split spherical head without a set; the mesh before the onsets; nothing of it without align"""
    calls = []
    ctx = types.SimpleNamespace(cfg=types.SimpleNamespace(sample_rate=FS),
                                hrtf_set=lambda dirs, hrir: calls.append(("set", np.array(dirs), np.array(hrir))),
                                hrtf_set_mesh=lambda tri: calls.append(("mesh", np.array(tri))),
                                hrtf_set_onsets=lambda onsets: calls.append(("onsets", np.array(onsets))))
    plug = object.__new__(pkg.FrequenSeeAudioBinauralPlugin)
    plug.ctx = ctx
    rng = np.random.default_rng(3)
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    hrir, _ = planted(rng, 6, 32)

    plug.SetHrtf(dirs, hrir, interpolate=True, align=True)
    assert [c[0] for c in calls] == ["set", "mesh", "onsets"]
    aligned, onsets = pkg.Context.hrtf_split_onsets(hrir, 0.1, 0)
    assert calls[0][2].tobytes() == aligned.tobytes() and calls[2][1].tobytes() == onsets.tobytes() and calls[1][1].shape == (8, 3)
    calls.clear()
    mine = rng.uniform(0, 5, (6, 2)).astype(np.float32)
    plug.SetHrtf(dirs, hrir, align=True, onsets=mine)
    assert [c[0] for c in calls] == ["set", "onsets"] and calls[0][2].tobytes() == hrir.tobytes() and calls[1][1].tobytes() == mine.tobytes()
    calls.clear()
    plug.SetHrtf(directions=64, taps=16, interpolate=True, align=True)
    d, g, o = pkg.Context.hrtf_spherical_head_split(FS, 64, 16)
    assert [c[0] for c in calls] == ["set", "mesh", "onsets"]
    assert calls[0][1].tobytes() == d.tobytes() and calls[0][2].tobytes() == g.tobytes() and calls[2][1].tobytes() == o.tobytes()
    calls.clear()
    for kw in (dict(dirs=dirs, hrir=hrir, onsets=mine), dict(onsets=mine, align=True), dict(dirs=dirs, hrir=hrir, align=True, onsets=mine[:5])):
        with pytest.raises(ValueError):   # onsets without align, without a set, of another shape: refused before any library call
            plug.SetHrtf(**kw)
    assert not calls
    plug.SetHrtf(dirs, hrir, interpolate=True)
    plug.SetHrtf(directions=64, taps=64)
    assert [c[0] for c in calls] == ["set", "mesh", "set"] and calls[0][2].tobytes() == hrir.tobytes()
    assert calls[2][2].tobytes() == pkg.Context.hrtf_spherical_head(FS, 64, 64)[1].tobytes()
