#!/usr/bin/env python3
"""Early-reflection timing: the median host wall time of one fs_reflection_render_process_batch call (1024 stereo frames per source,
8 bands, T = 255, every voice's delay and gains ramping, the copies up and back and the stream wait included, mix requested) for
{1, 32, 256} sources x {4, 16} voices.  Beside it, in the same process: fs_direct_render_process_batch with sources x voices rows
(where that fits under 256 rows) — one direct "source" per reflection, the workaround the voice bank replaces — and a plain direct
batch of the same source count.  The C entry points are called with prepared arrays: the numbers are the library's, not the Python
wrapper's.
usage: python tools/measure_reflection_render.py [reps] [output.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

FRAME, TAPS, BANDS, SOURCES, VOICES, MAX_ROWS = 1024, 255, 8, (1, 32, 256), (4, 16), 256
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
bank = [ctx.create_source() for _ in range(max(SOURCES))]
rows_src = [ctx.create_source() for _ in range(MAX_ROWS)]
for s in rows_src:
    ctx.direct_render_init(s, FRAME, TAPS, 0.1)
blocks = rng.uniform(-1, 1, (MAX_ROWS, 2 * FRAME)).astype(np.float32)
out = np.empty_like(blocks)
mix = np.empty(2 * FRAME, np.float32)


def handles(srcs):
    return np.ascontiguousarray(srcs, dtype=np.int32)


def direct_ms(n, repeat_blocks_of):
    """n direct rows; row r gets the block of source r // repeat_blocks_of, as the workaround has to upload it"""
    h = handles(rows_src[:n])
    blk = np.ascontiguousarray(blocks[np.arange(n) // repeat_blocks_of])
    tg = [np.zeros(n, dtype=pkg.Context.RENDER_TARGET_DTYPE) for _ in range(2)]
    tg[0]["delay"] = rng.uniform(0.0, 0.05, n)
    tg[1]["delay"] = tg[0]["delay"] + 0.004
    for t in tg:
        t["band_gain"] = rng.uniform(0.0, 1.0, (n, 8))
    flip = [0]

    def call():   # the targets alternate: every callback ramps delay and gains
        flip[0] ^= 1
        rc = lib.fs_direct_render_process_batch(ctx.h, h.ctypes.data, n, blk.ctypes.data, tg[flip[0]].ctypes.data, out.ctypes.data, mix.ctypes.data)
        assert rc == cap.OK, rc

    return median_ms(call)


result = {"callback": f"{FRAME} stereo frames per source, {BANDS} bands, T = {TAPS}", "reps": reps, "realtime_budget_ms": FRAME / 48.0, "rows": []}
for voices in VOICES:
    for s in bank:
        ctx.reflection_render_init(s, FRAME, TAPS, voices, 0.1)
    for n in SOURCES:
        h = handles(bank[:n])
        counts = np.full(n, voices, np.int32)
        vo = [np.zeros((n, voices), dtype=pkg.Context.REFLECTION_VOICE_DTYPE) for _ in range(2)]
        vo[0]["delay"] = rng.uniform(0.0, 0.05, (n, voices))
        vo[1]["delay"] = vo[0]["delay"] + 0.004
        for v in vo:
            v["key"] = np.arange(voices, dtype=np.uint32)[None, :]
            v["band_gain"] = rng.uniform(0.0, 1.0, (n, voices, 8))
            v["channel_gain"] = rng.uniform(-1.0, 1.0, (n, voices, 2))
        blk = np.ascontiguousarray(blocks[:n])
        rows = np.zeros(n, dtype=pkg.Context.REFLECTION_RENDER_ROW_DTYPE)
        flip = [0]

        def call():   # the entries alternate: every voice continues and ramps its delay and all its gains
            flip[0] ^= 1
            rc = lib.fs_reflection_render_process_batch(ctx.h, h.ctypes.data, n, blk.ctypes.data, vo[flip[0]].ctypes.data, counts.ctypes.data,
                                                        voices, out.ctypes.data, mix.ctypes.data, rows.ctypes.data)
            assert rc == cap.OK, rc

        ms = median_ms(call)
        assert int(rows["sounding"].min()) == voices and int(rows["dropped"].max()) == 0
        row = {"sources": n, "voices": voices, "reflection_render_ms": ms, "macs": n * voices * TAPS * 2 * FRAME,
               "workaround_direct_rows": n * voices if n * voices <= MAX_ROWS else None,
               "workaround_direct_ms": direct_ms(n * voices, voices) if n * voices <= MAX_ROWS else None,
               "plain_direct_ms": direct_ms(n, 1)}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
# the workaround at 16 sources x 16 voices = 256 direct rows, and the bank at the same load
for s in bank[:16]:
    ctx.reflection_render_init(s, FRAME, TAPS, 16, 0.1)
h16 = handles(bank[:16])
v16 = [np.zeros((16, 16), dtype=pkg.Context.REFLECTION_VOICE_DTYPE) for _ in range(2)]
v16[0]["delay"] = rng.uniform(0.0, 0.05, (16, 16))
v16[1]["delay"] = v16[0]["delay"] + 0.004
for v in v16:
    v["key"] = np.arange(16, dtype=np.uint32)[None, :]
    v["band_gain"] = rng.uniform(0.0, 1.0, (16, 16, 8))
    v["channel_gain"] = rng.uniform(-1.0, 1.0, (16, 16, 2))
c16 = np.full(16, 16, np.int32)
b16 = np.ascontiguousarray(blocks[:16])
flip16 = [0]


def call16():
    flip16[0] ^= 1
    rc = lib.fs_reflection_render_process_batch(ctx.h, h16.ctypes.data, 16, b16.ctypes.data, v16[flip16[0]].ctypes.data, c16.ctypes.data, 16,
                                                out.ctypes.data, mix.ctypes.data, None)
    assert rc == cap.OK, rc


bank16, rows256 = median_ms(call16), direct_ms(256, 16)
result["sixteen_by_sixteen"] = {"reflection_render_ms": bank16, "workaround_direct_256_rows_ms": rows256, "ratio": rows256 / bank16}
print(json.dumps(result["sixteen_by_sixteen"]), flush=True)
ctx.close()
text = json.dumps(result)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
