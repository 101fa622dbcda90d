#!/usr/bin/env python3
"""Row f2 with fs_reverb_set_crossfade: what the crossfade costs the audio callback and what it does to the output.

  * host time per fs_reverb_process call (1024 stereo frames, 48 000-tap IR; includes the 8 KB round trip and the stream
    sync the audio thread waits for), averaged over --callbacks calls per mode after a warm-up, the modes alternating in
    rounds: crossfade off; on (2560 samples) with a constant IR; on with a new IR (fs_set_impulse_response) before every
    callback — the install itself is not timed;
  * the largest step |y[0] - y_prev[last]| at block boundaries on a steady 220 Hz sine, without and with the fade, with a new
    traced IR (1000 pairs, starter_room) before every callback, beside the largest step inside the blocks.

--profile-run: only a short loop of plain and fading callbacks, for `rocprofv3 --kernel-trace --stats` (kernel times).
usage: python tools/measure_reverb_crossfade.py [--callbacks 2000] [--out FILE.json] | --profile-run"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

FRAME = 1024
FADE = 2560


def noise_ir(rng, n):
    return (rng.normal(0, 1, n) * np.exp(-np.arange(n) / 5000.0) * 0.02).astype(np.float32)


def callback_times(pkg, callbacks, rounds=4):
    ctx = pkg.Context(num_bands=1)
    n = ctx.num_samples
    rng = np.random.default_rng(0)
    modes = {"off": ctx.create_source(np.zeros(3, np.float32)), "on_constant_ir": ctx.create_source(np.zeros(3, np.float32)),
             "on_new_ir_every_callback": ctx.create_source(np.zeros(3, np.float32))}
    irs = [noise_ir(rng, n) for _ in range(8)]
    for name, s in modes.items():
        ctx.reverb_init(s, FRAME)
        if name != "off":
            ctx.reverb_set_crossfade(s, FADE)
        ctx.set_impulse_response(s, irs[0])
    blk = np.clip(rng.normal(0, 0.3, 2 * FRAME), -1, 1).astype(np.float32)
    lib, h = ctx.lib, ctx.h
    out = np.empty_like(blk)
    total = {k: 0.0 for k in modes}
    count = {k: 0 for k in modes}
    per = (callbacks + rounds - 1) // rounds
    for r in range(rounds + 1):                       # round 0: warm-up, not counted
        for name, s in modes.items():
            for i in range(per if r else 50):
                if name == "on_new_ir_every_callback":
                    ctx.set_impulse_response(s, irs[i % len(irs)])
                t = time.perf_counter()
                rc = lib.fs_reverb_process(h, s, blk.ctypes.data, out.ctypes.data, 1, 0)
                dt = time.perf_counter() - t
                ctx.check(rc)
                if r:
                    total[name] += dt
                    count[name] += 1
    ctx.close()
    ms = {k: 1e3 * total[k] / count[k] for k in modes}
    return ms, count


def boundary_steps(pkg, callbacks=120):
    sc = pkg.scenes.starter_room(4)
    ctx = pkg.Context(num_bands=4)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    tracer = ctx.create_source(sc.source)
    plain, fade = ctx.create_source(sc.source), ctx.create_source(sc.source)
    for s in (plain, fade):
        ctx.reverb_init(s, FRAME)
    ctx.reverb_set_crossfade(fade, FRAME)
    t = np.arange(FRAME * (callbacks + 1)) / 48000.0
    sine = (0.5 * np.sin(2 * np.pi * 220.0 * t)).astype(np.float32)
    prev = {plain: None, fade: None}
    res = {plain: {"boundary": [], "inside": 0.0}, fade: {"boundary": [], "inside": 0.0}}
    for c in range(callbacks):
        ctx.update_sources([tracer], pkg.default_params(num_rays=2000, depth=8, seed=500 + c, dist_divisor=100.0))
        ir = ctx.impulse_response(tracer, 0)
        blk = np.repeat(sine[c * FRAME:(c + 1) * FRAME], 2)
        for s in (plain, fade):
            ctx.set_impulse_response(s, ir)
            y = ctx.reverb_process(s, blk)[0::2].astype(np.float64)
            if prev[s] is not None and c >= 50:            # (after the first 1 s: the history is full)
                res[s]["boundary"].append(abs(y[0] - prev[s][-1]))
                res[s]["inside"] = max(res[s]["inside"], float(np.abs(np.diff(y)).max()))
            prev[s] = y
    ctx.close()
    return {name: {"largest_boundary_step": float(max(r["boundary"])), "mean_boundary_step": float(np.mean(r["boundary"])),
                   "largest_step_inside_blocks": r["inside"], "boundaries": len(r["boundary"])}
            for name, r in (("abrupt_switch", res[plain]), (f"crossfade_{FRAME}", res[fade]))}


def profile_run(pkg, callbacks=200):
    ctx = pkg.Context(num_bands=1)
    rng = np.random.default_rng(1)
    a, b = ctx.create_source(np.zeros(3, np.float32)), ctx.create_source(np.zeros(3, np.float32))
    for s in (a, b):
        ctx.reverb_init(s, FRAME)
    ctx.reverb_set_crossfade(b, FADE)                     # a new IR every callback: b is fading in every one of them
    blk = np.clip(rng.normal(0, 0.3, 2 * FRAME), -1, 1).astype(np.float32)
    irs = [noise_ir(rng, ctx.num_samples) for _ in range(4)]
    for i in range(callbacks):
        ctx.set_impulse_response(a, irs[i % 4])
        ctx.set_impulse_response(b, irs[i % 4])
        ctx.reverb_process(a, blk)
        ctx.reverb_process(b, blk)
    ctx.close()
    print(json.dumps({"profile_run": callbacks}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--callbacks", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    pkg = graft.load_package()
    if a.profile_run:
        profile_run(pkg)
        return 0
    ms, count = callback_times(pkg, a.callbacks)
    rec = {"callback": "1024 stereo frames, 48000-tap IR, crossfade 2560 samples", "ms_per_callback": ms, "callbacks_timed": count,
           "on_constant_over_off": ms["on_constant_ir"] / ms["off"], "new_ir_over_off": ms["on_new_ir_every_callback"] / ms["off"],
           "steps_220Hz_sine_traced_1000_pair_irs": boundary_steps(pkg)}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
