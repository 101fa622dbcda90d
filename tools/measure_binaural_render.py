#!/usr/bin/env python3
"""Binaural-voice timing: the median host wall time of one fs_binaural_render_process_batch call (1024 stereo frames per source,
8 bands, T = 255, a spherical-head set of 1024 directions and H = 128 taps, every voice's delay, gains and direction ramping in
every callback, the copies up and back and the stream wait included, mix requested) for {1, 32, 256} sources x {4, 16} voices.
Beside it, in the same process and at the same shapes: fs_reflection_render_process_batch, which the binaural renderer is with a
gain pair in the HRIRs' place.  The C entry points are called with prepared arrays: the numbers are the library's, not the Python
wrapper's.  With --interpolate the set carries its mesh (fs_hrtf_triangulate, fs_hrtf_set_mesh: 2044 triangles) and every voice's HRIR
is the blend of three: the same shapes, one more launch (the locate pass).
With --onsets the set is the split spherical head (fs_hrtf_spherical_head_split, fs_hrtf_set_onsets), with or without --interpolate:
every voice's HRIR is the aligned one delayed by the voice's own onset, He = H + (int)omax + 1 taps; --hrir-taps=N sets H (the split
head at H = 96 has the He = 128 of the plain head's table).
--directions=N measures a set of another size (the table's is 1024).
usage: python tools/measure_binaural_render.py [--interpolate] [--onsets] [--hrir-taps=N] [--directions=N] [reps] [output.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

FRAME, TAPS, BANDS, HRIR_TAPS, DIRECTIONS, SOURCES, VOICES = 1024, 255, 8, 128, 1024, (1, 32, 256), (4, 16)
INTERPOLATE = "--interpolate" in sys.argv
ONSETS = "--onsets" in sys.argv
for a in sys.argv:
    if a.startswith("--directions="):
        DIRECTIONS = int(a.split("=", 1)[1])
    if a.startswith("--hrir-taps="):
        HRIR_TAPS = int(a.split("=", 1)[1])
sys.argv = [a for a in sys.argv if not a.startswith("--")]
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
pkg = graft.load_package()
cap = pkg._capi
lib = cap.load()
rng = np.random.default_rng(0)


def median_ms(call):
    for _ in range(10):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


ctx = pkg.Context(num_bands=BANDS)
if ONSETS:
    the_set = pkg.Context.hrtf_spherical_head_split(ctx.cfg.sample_rate, DIRECTIONS, HRIR_TAPS)
else:
    the_set = pkg.Context.hrtf_spherical_head(ctx.cfg.sample_rate, DIRECTIONS, HRIR_TAPS)
ctx.hrtf_set(*the_set[:2])
if INTERPOLATE:
    ctx.hrtf_set_mesh(pkg.Context.hrtf_triangulate(the_set[0]))
EXTRA_TAPS = 0
if ONSETS:
    ctx.hrtf_set_onsets(the_set[2])
    EXTRA_TAPS = ctx.hrtf_onsets_info()[1]
binaural = [ctx.create_source() for _ in range(max(SOURCES))]
reflect = [ctx.create_source() for _ in range(max(SOURCES))]
blocks = rng.uniform(-1, 1, (max(SOURCES), 2 * FRAME)).astype(np.float32)
out = np.empty_like(blocks)
mix = np.empty(2 * FRAME, np.float32)
result = {"callback": f"{FRAME} stereo frames per source, {BANDS} bands, T = {TAPS}, H = {HRIR_TAPS}, {DIRECTIONS} directions", "reps": reps,
          "mode": ("interpolated" if INTERPOLATE else "nearest") + (" with onsets" if ONSETS else ""), "delayed_hrir_taps": HRIR_TAPS + EXTRA_TAPS,
          "triangles": ctx.hrtf_mesh_info(), "realtime_budget_ms": FRAME / 48.0, "rows": []}
for voices in VOICES:
    for s in binaural:
        ctx.binaural_render_init(s, FRAME, TAPS, voices, 0.1)
    for s in reflect:
        ctx.reflection_render_init(s, FRAME, TAPS, voices, 0.1)
    for n in SOURCES:
        hb = np.ascontiguousarray(binaural[:n], dtype=np.int32)
        hr = np.ascontiguousarray(reflect[:n], dtype=np.int32)
        counts = np.full(n, voices, np.int32)
        bv = [np.zeros((n, voices), dtype=pkg.Context.BINAURAL_VOICE_DTYPE) for _ in range(2)]
        rv = [np.zeros((n, voices), dtype=pkg.Context.REFLECTION_VOICE_DTYPE) for _ in range(2)]
        delay = rng.uniform(0.0, 0.05, (n, voices))
        for k in range(2):   # the two lists a callback alternates between: every voice continues and ramps everything it has
            for v in (bv[k], rv[k]):
                v["key"] = np.arange(voices, dtype=np.uint32)[None, :]
                v["delay"] = delay + 0.004 * k
                v["band_gain"] = rng.uniform(0.0, 1.0, (n, voices, 8))
            bv[k]["gain"] = rng.uniform(-1.0, 1.0, (n, voices))
            bv[k]["direction"] = rng.normal(size=(n, voices, 3))
            rv[k]["channel_gain"] = rng.uniform(-1.0, 1.0, (n, voices, 2))
        blk = np.ascontiguousarray(blocks[:n])
        brows = np.zeros(n, dtype=pkg.Context.BINAURAL_RENDER_ROW_DTYPE)
        rrows = np.zeros(n, dtype=pkg.Context.REFLECTION_RENDER_ROW_DTYPE)
        flip = [0, 0]

        def binaural_call():
            flip[0] ^= 1
            rc = lib.fs_binaural_render_process_batch(ctx.h, hb.ctypes.data, n, blk.ctypes.data, bv[flip[0]].ctypes.data, counts.ctypes.data,
                                                      voices, out.ctypes.data, mix.ctypes.data, brows.ctypes.data)
            assert rc == cap.OK, rc

        def reflection_call():
            flip[1] ^= 1
            rc = lib.fs_reflection_render_process_batch(ctx.h, hr.ctypes.data, n, blk.ctypes.data, rv[flip[1]].ctypes.data, counts.ctypes.data,
                                                        voices, out.ctypes.data, mix.ctypes.data, rrows.ctypes.data)
            assert rc == cap.OK, rc

        b_ms, r_ms = median_ms(binaural_call), median_ms(reflection_call)
        for rows in (brows, rrows):
            assert int(rows["sounding"].min()) == voices and int(rows["dropped"].max()) == 0 and int(rows["started"].max()) == 0
        row = {"sources": n, "voices": voices, "mode": result["mode"], "binaural_render_ms": b_ms, "reflection_render_ms": r_ms, "ratio": b_ms / r_ms,
               "folded_taps": TAPS + HRIR_TAPS + EXTRA_TAPS - 1, "fits_the_block": b_ms <= FRAME / 48.0}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
ctx.close()
text = json.dumps(result)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
