"""Binaural voices, the part that needs no device: the exports and struct layouts, fs_hrtf_spherical_head against a numpy float64
restatement of the header's formula, its symmetry, its interaural delay, its unit DC gain and its refusals, and the component
layer's Voices() — the head-frame rotation and the direct sound's voice — on hand-made path records
(include/frequensee.h, "binaural voices on the audio thread")."""
import ctypes as C
import math
import os

import numpy as np
import pytest

F32 = np.float32
FS = 48000
EPS = 2.0 ** -24
A_CM, C_CM_S = 8.75, 34300.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fs_hrtf_set", "fs_hrtf_info", "fs_hrtf_spherical_head", "fs_binaural_render_init", "fs_binaural_render_release",
       "fs_binaural_render_process_batch")


def test_struct_and_exports(pkg):
    cap = pkg._capi
    V, R, D = cap.BinauralVoice, cap.BinauralRenderRow, cap.HrtfDesc
    assert C.sizeof(V) == 56 and C.sizeof(R) == 16 and C.sizeof(D) == 32
    assert (V.key.offset, V.delay.offset, V.band_gain.offset, V.gain.offset, V.direction.offset) == (0, 4, 8, 40, 44)
    assert (R.sounding.offset, R.started.offset, R.ended.offset, R.dropped.offset) == (0, 4, 8, 12)
    assert (D.struct_size.offset, D.directions.offset, D.taps.offset, D.sample_rate.offset, D.dirs.offset, D.hrir.offset) == (0, 4, 8, 12, 16, 24)
    vd, rd = pkg.Context.BINAURAL_VOICE_DTYPE, pkg.Context.BINAURAL_RENDER_ROW_DTYPE
    assert vd.itemsize == 56 and rd.itemsize == 16
    assert [vd.fields[k][1] for k in ("key", "delay", "band_gain", "gain", "direction")] == [0, 4, 8, 40, 44]
    assert (cap.MAX_HRTF_DIRECTIONS, cap.MAX_HRTF_TAPS, cap.BINAURAL_DIRECT_KEY) == (4096, 512, 0x1FFFFFFF)
    header = open(os.path.join(ROOT, "include", "frequensee.h")).read()
    for name in NEW:
        assert name in cap.EXPORTS and hasattr(cap.load(), name)
        assert name in header[:header.index("#ifndef FREQUENSEE_H")], f"{name} is not in the header's export list"
    assert cap.load().fs_abi_version() == 5
    assert "FrequenSeeAudioBinauralPlugin" in pkg.__all__


def test_null_context_and_no_device(pkg):
    cap = pkg._capi
    lib = cap.load()
    n, H = C.c_int32(7), C.c_int32(7)
    dirs, hrir = pkg.Context.hrtf_spherical_head(FS, 6, 40)
    desc = cap.HrtfDesc(C.sizeof(cap.HrtfDesc), 6, 40, FS, dirs.ctypes.data, hrir.ctypes.data)
    assert lib.fs_hrtf_set(None, C.byref(desc)) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_hrtf_info(None, C.byref(n), C.byref(H)) == cap.ERR_INVALID_ARGUMENT and (n.value, H.value) == (7, 7)
    assert lib.fs_binaural_render_init(None, 0, 64, 15, 4, 0.01) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_binaural_render_release(None, 0) == cap.ERR_INVALID_ARGUMENT
    src = (C.c_int32 * 1)(0)
    cnt = (C.c_int32 * 1)(1)
    blk = np.zeros(128, np.float32)
    out = np.full(128, 7.0, np.float32)
    rows = np.full(4, 7, np.uint32)
    vo = np.zeros(1, dtype=pkg.Context.BINAURAL_VOICE_DTYPE)
    call = lib.fs_binaural_render_process_batch
    assert call(None, src, 1, blk.ctypes.data, vo.ctypes.data, cnt, 1, out.ctypes.data, None, rows.ctypes.data) == cap.ERR_INVALID_ARGUMENT
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        cfg = cap.default_config(num_bands=1)
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == cap.ERR_NO_DEVICE and h
        try:
            assert lib.fs_hrtf_set(h, C.byref(desc)) == cap.ERR_NO_DEVICE
            assert lib.fs_hrtf_info(h, C.byref(n), C.byref(H)) == cap.OK and (n.value, H.value) == (0, 0)
            assert lib.fs_binaural_render_init(h, 0, 64, 15, 4, 0.01) == cap.ERR_NO_DEVICE
            assert b"no CPU fallback" in lib.fs_last_error(h)
            assert call(h, src, 1, blk.ctypes.data, vo.ctypes.data, cnt, 1, out.ctypes.data, None, rows.ctypes.data) == cap.ERR_NO_DEVICE
            assert call(h, src, 1, blk.ctypes.data, vo.ctypes.data, cnt, 1, None, None, rows.ctypes.data) == cap.ERR_INVALID_ARGUMENT
        finally:
            lib.fs_context_destroy(h)
    assert np.all(out == 7.0) and np.all(rows == 7)


# ---- the spherical head: the header's formula in numpy double ---------------------------------------------------------------
def head_dirs64(n):
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def ear_taps64(dot, fs, H, a=A_CM, c=C_CM_S):
    """one ear's h[0 .. H) for p . e = dot"""
    theta = math.acos(min(max(dot, -1.0), 1.0))
    tau = (a / c) * (1.0 - math.cos(theta)) if theta <= math.pi / 2 else (a / c) * (1.0 + theta - math.pi / 2)
    alpha_min, theta_min = 0.1, 5.0 * math.pi / 6.0
    alpha = (1.0 + alpha_min / 2.0) + (1.0 - alpha_min / 2.0) * math.cos(theta * math.pi / theta_min)
    kappa = fs * (a / c)
    b0, b1, a1 = (1.0 + alpha * kappa) / (1.0 + kappa), (1.0 - alpha * kappa) / (1.0 + kappa), (1.0 - kappa) / (1.0 + kappa)
    g = np.zeros(H + 1)
    g[0] = b0
    if H >= 1:
        g[1] = b1 - a1 * g[0]
    for m in range(2, H + 1):
        g[m] = -a1 * g[m - 1]
    i = math.floor(tau * fs)
    f = tau * fs - i
    h = np.zeros(H)
    for k in range(H):
        m = k - i
        h[k] = (1.0 - f) * (g[m] if m >= 0 else 0.0) + f * (g[m - 1] if m >= 1 else 0.0)
    return h


def head64(fs, n, H):
    p = head_dirs64(n)
    return p, np.stack([np.stack([ear_taps64(-p[k, 1], fs, H), ear_taps64(p[k, 1], fs, H)]) for k in range(n)])


def within_one_ulp(got, ref):
    ulp = np.maximum(np.spacing(np.abs(ref.astype(np.float32))), np.spacing(np.abs(got))).astype(np.float64)
    return np.all(np.abs(got.astype(np.float64) - ref) <= ulp)


@pytest.mark.parametrize("fs,n,H", [(48000, 1, 40), (48000, 6, 64), (48000, 258, 128), (48000, 6, 40), (48000, 258, 64), (16000, 6, 24), (16000, 258, 24)])
def test_spherical_head_against_the_formula(pkg, fs, n, H):
    """the tolerance of the band kernels' test: one float32 ulp from the float64 formula"""
    dirs, hrir = pkg.Context.hrtf_spherical_head(fs, n, H)
    assert dirs.shape == (n, 3) and hrir.shape == (n, 2, H) and dirs.dtype == hrir.dtype == np.float32
    p, h = head64(fs, n, H)
    assert within_one_ulp(dirs, p), "a direction more than 1 float32 ulp from the formula"
    assert within_one_ulp(hrir, h), "a tap more than 1 float32 ulp from the formula"
    assert np.all(np.abs((dirs.astype(np.float64) ** 2).sum(1) - 1.0) <= 1e-6), "unit vectors: fs_hrtf_set's 1e-3 is far"
    assert np.isfinite(hrir).all()


def test_spherical_head_is_mirror_symmetric(pkg):
    """an ear's taps depend on the direction through p . e alone, e = (0, -+1, 0): the left HRIR of p is the right HRIR of p
    mirrored in y.  The call writes its own directions and the spiral holds no two that mirror each other, so bit for bit this can
    be checked only where a direction is its own mirror image (y == 0: k = 0 of every set, and the n = 1 set): both ears are equal
    there.  For y != 0 what is checked is the weaker consequence: on either side of the head the far ear is the weaker one."""
    dirs, hrir = pkg.Context.hrtf_spherical_head(FS, 258, 64)
    assert dirs[0, 1] == 0.0 and hrir[0, 0].tobytes() == hrir[0, 1].tobytes() and hrir[0, 0].any()
    one_dir, one_hrir = pkg.Context.hrtf_spherical_head(FS, 1, 64)   # n = 1: (1, 0, 0)
    assert np.array_equal(one_dir, [[1.0, 0.0, 0.0]]) and one_hrir[0, 0].tobytes() == one_hrir[0, 1].tobytes()
    # theta = acos(-+y): with y -> -y the two ears' angles swap, so on the side of the head (|y| large) the far ear is later and weaker
    right = int(np.argmax(dirs[:, 1]))
    left = int(np.argmin(dirs[:, 1]))
    assert np.abs(hrir[right, 1]).max() > np.abs(hrir[right, 0]).max() and np.abs(hrir[left, 0]).max() > np.abs(hrir[left, 1]).max()


def test_spherical_head_interaural_delay(pkg):
    """from +y the right ear hears at once (theta = 0: tau = 0) and the left after the longest way round, (a / c)(pi / 2 + 1) fs =
    31.48 samples at 48 kHz: the first non-zero taps lie that far apart, within one sample.  The set's nearest direction lies an
    angle delta off +y, which takes kappa delta = 12.2 delta samples off the left ear's onset (and puts kappa (1 - cos delta) on the
    right's), and a tap index is whole; so the set is the densest one, n = 4096, whose nearest direction is within 0.03 rad."""
    dirs, hrir = pkg.Context.hrtf_spherical_head(FS, 4096, 64)
    k = int(np.argmax(dirs[:, 1]))
    delta = math.acos(float(dirs[k, 1]))
    first = [int(np.nonzero(hrir[k, ear])[0][0]) for ear in range(2)]
    want = (A_CM / C_CM_S) * (math.pi / 2 + 1.0) * FS
    print(f"nearest +y at {delta:.4f} rad: first taps left {first[0]} right {first[1]}, the model's lag {want:.2f}")
    assert delta <= 0.03
    assert first[1] == 0 and abs((first[0] - first[1]) - want) <= 1.0


def test_spherical_head_sums_to_one(pkg):
    """The filter's DC gain is ((1 + alpha kappa) + (1 - alpha kappa)) / ((1 + kappa) + (1 - kappa)) = 1 and the fractional delay's
    two weights sum to 1, so sum_k h[k] = 1 less the truncated tail.  For m >= 1, g[m] = g[1] p^(m-1) with the pole p = -(1 - kappa) /
    (1 + kappa) and g[1] = b1 - a1 b0 = 2 kappa (1 - alpha) / (1 + kappa)^2, so sum_{m > N} g[m] = g[1] p^N / (1 - p) = kappa (1 - alpha)
    p^N / (1 + kappa), of magnitude <= |p|^N because 0.1 <= alpha <= 2.  The taps hold g up to N >= H - 2 - i_max at least, i_max =
    floor((a / c)(1 + pi / 2) fs) the latest onset.  Each tap (|h| <= 2) is rounded to float once: H 2^-24 2 more."""
    H = 128
    dirs, hrir = pkg.Context.hrtf_spherical_head(FS, 258, H)
    kappa = FS * A_CM / C_CM_S
    pole = abs((1.0 - kappa) / (1.0 + kappa))
    i_max = math.floor((A_CM / C_CM_S) * (1.0 + math.pi / 2) * FS)
    bound = pole ** (H - 2 - i_max) + 2 * H * EPS
    worst = float(np.abs(hrir.astype(np.float64).sum(axis=2) - 1.0).max())
    print(f"|sum h - 1| <= {worst:.3e}, bound {bound:.3e} (pole {pole:.4f}, i_max {i_max})")
    assert worst <= bound
    assert np.abs(hrir).max() <= 2.0


def test_spherical_head_refusals(pkg):
    cap = pkg._capi
    lib = cap.load()
    dirs, hrir = np.full((6, 3), 7.0, np.float32), np.full((6, 2, 64), 7.0, np.float32)
    d, h = dirs.ctypes.data, hrir.ctypes.data
    nan, inf = float("nan"), float("inf")

    def call(fs=FS, a=A_CM, c=C_CM_S, n=6, H=64, dp=d, hp=h):
        return lib.fs_hrtf_spherical_head(fs, C.c_float(a), C.c_float(c), n, H, dp, hp)

    need = math.ceil((A_CM / C_CM_S) * (1.0 + math.pi / 2) * FS) + 2
    assert need == 34
    bad = [dict(fs=0), dict(fs=-1), dict(a=0.0), dict(a=-1.0), dict(a=nan), dict(a=inf), dict(c=0.0), dict(c=-343.0), dict(c=nan), dict(c=inf),
           dict(n=0), dict(n=-1), dict(n=4097), dict(H=0), dict(H=-1), dict(H=513), dict(H=need - 1), dict(dp=None), dict(hp=None),
           dict(a=100.0, H=64)]   # a head of one metre: the onset alone is 360 samples
    for kw in bad:
        assert call(**kw) == cap.ERR_INVALID_ARGUMENT, kw
    assert np.all(dirs == 7.0) and np.all(hrir == 7.0), "a refused call wrote"
    small = np.zeros((6, 2, need), np.float32)
    assert call(H=need, hp=small.ctypes.data) == cap.OK, "the least H the header accepts"
    with pytest.raises(pkg.FrequenSeeError):
        pkg.Context.hrtf_spherical_head(FS, 6, need - 1)
    big_d, big_h = pkg.Context.hrtf_spherical_head(FS, 4096, 34)
    assert big_d.shape == (4096, 3) and np.isfinite(big_h).all()


# ---- the component layer -------------------------------------------------------------------------------------------------------
class _Ctx:   # what Voices() reads of a context
    class cfg:
        sample_rate = FS


def _plug(pkg, taps=255):
    plug = pkg.FrequenSeeAudioBinauralPlugin.__new__(pkg.FrequenSeeAudioBinauralPlugin)
    plug.ctx, plug.Taps = _Ctx, taps
    return plug


def test_voices_head_frame_and_gain(pkg):
    plug = _plug(pkg)
    paths = np.zeros(4, dtype=pkg.Context.REFLECTION_DTYPE)
    row = np.zeros(1, dtype=pkg.Context.REFLECTION_ROW_DTYPE)[0]
    paths["direction"] = [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8]]
    paths["triangle"] = [11, 5, 2, 99]
    paths["delay"] = [0.01, 0.001, 0.02, 0.03]   # 0.001 s is less than the latency of 127 samples
    paths["length"] = [200.0, 50.0, 400.0, 800.0]
    paths["reflectance"] = np.arange(32, dtype=np.float32).reshape(4, 8) / 32
    row["returned"] = 3
    v = plug.Voices(row, paths, forward=[1.0, 0.0, 0.0], right=[0.0, 1.0, 0.0])
    assert v.dtype == pkg.Context.BINAURAL_VOICE_DTYPE and v.shape == (3,), "only the returned paths become entries"
    assert list(v["key"]) == [11, 5, 2]
    assert np.array_equal(v["band_gain"], paths["reflectance"][:3])
    latency = 127 / FS
    assert v["delay"][0] == F32(float(F32(0.01)) - latency) and v["delay"][1] == 0.0 and v["delay"][2] == F32(float(F32(0.02)) - latency)
    assert np.array_equal(v["gain"], np.ones(3, np.float32))
    assert np.array_equal(v["direction"], paths["direction"][:3]), "forward = +x, right = +y gives up = +z: the identity"
    near = plug.Voices(row, paths, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], reference_length=100.0)   # min(1, 100 / length)
    assert np.array_equal(near["gain"], np.array([0.5, 1.0, 0.25], np.float32))
    # the listener turned a quarter to the left: forward = -y, right = +x, up = f x r = (f.y r.z - f.z r.y, f.z r.x - f.x r.z, f.x r.y - f.y r.x) = +z
    row["returned"] = 4
    t = plug.Voices(row, paths, forward=[0.0, -1.0, 0.0], right=[1.0, 0.0, 0.0])
    assert np.array_equal(t["direction"], np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.6, 0.8]], np.float32))
    # looking straight up, the right ear still to +y: forward = +z, right = +y, up = (0 * 0 - 1 * 1, 1 * 0 - 0 * 0, 0) = -x
    u = plug.Voices(row, paths, forward=[0.0, 0.0, 1.0], right=[0.0, 1.0, 0.0])
    assert np.array_equal(u["direction"], np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.8, 0.0, -0.6]], np.float32))
    row["returned"] = 0
    assert plug.Voices(row, paths, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]).shape == (0,)


def test_voices_direct_sound_and_the_other_kinds(pkg):
    plug = _plug(pkg, taps=15)
    paths = np.zeros(2, dtype=pkg.Context.REFLECTION_DTYPE)
    row = np.zeros(1, dtype=pkg.Context.REFLECTION_ROW_DTYPE)[0]
    paths["direction"] = [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]
    paths["triangle"] = [4, 9]
    paths["delay"] = [0.01, 0.02]
    paths["length"] = [343.0, 686.0]
    paths["reflectance"] = 0.5
    row["returned"] = 2
    direct = np.zeros(1, dtype=pkg.Context.DIRECT_DTYPE)[0]
    direct["delay"], direct["distance"] = 0.005, 200.0
    direct["transmission"] = np.arange(8, dtype=np.float32) / 8
    diff_paths = np.zeros(1, dtype=pkg.Context.DIFFRACTION_DTYPE)
    diff_row = np.zeros(1, dtype=pkg.Context.DIFFRACTION_ROW_DTYPE)[0]
    diff_paths["triangle"], diff_paths["edge"], diff_paths["delay"], diff_paths["length"] = 7, 2, 0.03, 1000.0
    diff_paths["direction"] = [[0.0, 0.0, -1.0]]
    diff_paths["gain"] = 0.25
    diff_row["returned"] = 1
    fwd, right = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    v = plug.Voices(row, paths, fwd, right, reference_length=100.0, direct=(direct, [0.0, -300.0, 0.0]), diffraction=(diff_row, diff_paths))
    assert list(v["key"]) == [0x1FFFFFFF, 4, 9, 0x80000000 | (4 * 7 + 2)], "the direct sound first, then the reflection plugin's order and keys"
    assert pkg.FrequenSeeAudioBinauralPlugin.DirectKey == pkg._capi.BINAURAL_DIRECT_KEY == 0x1FFFFFFF
    assert np.array_equal(v["band_gain"][0], direct["transmission"]) and np.all(v["band_gain"][3] == 0.25)
    assert v["delay"][0] == F32(float(F32(0.005)) - 7 / FS)
    assert np.array_equal(v["direction"][0], np.array([0.0, -300.0, 0.0], np.float32)), "from the listener to the source, any length"
    assert np.array_equal(v["direction"][3], np.array([0.0, 0.0, -1.0], np.float32))
    assert np.array_equal(v["gain"], np.array([0.5, 100.0 / 343.0, 100.0 / 686.0, 0.1], np.float32))
    # the same keys, delays and band gains as the reflection plugin gives
    refl = pkg.FrequenSeeAudioReflectionPlugin.__new__(pkg.FrequenSeeAudioReflectionPlugin)
    refl.ctx, refl.Taps = _Ctx, 15
    w = refl.Voices(row, paths, diffraction=(diff_row, diff_paths))
    for field in ("key", "delay", "band_gain"):
        assert np.array_equal(v[field][1:], w[field])
    paths["triangle"][1] = 0x1FFFFFFF
    with pytest.raises(ValueError):
        plug.Voices(row, paths, fwd, right, direct=(direct, [1.0, 0.0, 0.0]))
    plug.Voices(row, paths, fwd, right)   # without a direct voice the key is free
