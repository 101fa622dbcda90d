#!/usr/bin/env python3
"""Direct-sound timing: the median wall time of one fs_direct_render_process_batch call (1024 stereo frames per source, the
copies up and back and the stream wait the audio thread needs included) for 1, 32 and 256 sources at T = 255 and T = 2047, and
beside it fs_reverb_process_batch (direct engine, 48 000-tap IR) at the same counts on the same machine.
usage: python tests/measure_direct_render.py [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

FRAME, COUNTS, BANDS = 1024, (1, 32, 256), 8
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
pkg = graft.load_package()
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


out = {"callback": f"{FRAME} stereo frames per source", "reps": reps, "realtime_budget_ms": FRAME / 48.0, "rows": []}
ctx = pkg.Context(num_bands=BANDS)
srcs = [ctx.create_source() for _ in range(max(COUNTS))]
blocks = rng.uniform(-1, 1, (max(COUNTS), 2 * FRAME)).astype(np.float32)
targets = np.zeros(max(COUNTS), dtype=pkg.Context.RENDER_TARGET_DTYPE)
moving = targets.copy()
for i in range(max(COUNTS)):
    targets[i]["delay"] = rng.uniform(0.0, 0.05)
    targets[i]["band_gain"] = rng.uniform(0.0, 1.0, 8)
    moving[i]["delay"] = targets[i]["delay"] + 0.004
    moving[i]["band_gain"] = rng.uniform(0.0, 1.0, 8)
direct = {}
for taps in (255, 2047):
    for s in srcs:
        ctx.direct_render_init(s, FRAME, taps, 0.1)
    for n in COUNTS:
        flip = [0]

        def call(n=n):   # the targets alternate: every callback ramps delay and gains
            flip[0] ^= 1
            ctx.direct_render_process_batch(srcs[:n], blocks[:n], (moving if flip[0] else targets)[:n], want_mix=True)

        direct[(taps, n)] = median_ms(call)
ir = (rng.normal(0, 1, ctx.num_samples) * np.exp(-np.arange(ctx.num_samples) / 5000.0) * 0.02).astype(np.float32)
for s in srcs:
    ctx.reverb_init(s, FRAME)
    ctx.set_impulse_response(s, ir)
quiet = (blocks * np.float32(0.3)).astype(np.float32)
for n in COUNTS:
    reverb_ms = median_ms(lambda n=n: ctx.reverb_process_batch(srcs[:n], quiet[:n], want_mix=True))
    out["rows"].append({"count": n, "direct_render_ms_taps_255": direct[(255, n)], "direct_render_ms_taps_2047": direct[(2047, n)],
                        "reverb_direct_engine_ms": reverb_ms})
ctx.close()
print(json.dumps(out))
