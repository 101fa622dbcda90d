#!/usr/bin/env python3
"""Order window (fs_source_set_order_window): what a windowed source costs.

Three pieces of work, each in three modes that alternate in one process:
  plain   — no window, no table: the ordinary route;
  window  — the window (1, unbounded): the direct path is left out;
  allpass — no window, an all-ones directivity table: the cost the directional (EXT) connect route had before the window
            existed, and the yardstick for `window`.

  * a waited-for cfg3 frame: old_mine, 8 bands, 262 144 rays, depth 8 (fs_compute_energy_response);
  * a tick of 32 sources (fs_update_sources: 2 000 rays each, depth 0) on starter_room, every source in the mode;
  * a pipelined stream (fs_set_pipelining(2), two frames per launch) of 8 sources x 32 768 rays, depth 8, starter_room, in which
    one source is in the mode — its frames are not held, so they end the fused launches around them.

Host wall time per frame / tick (the work ends in a synchronise).  The repetitions are split into --rounds rounds; every round
gives one median per mode, the result is the median of the round medians, and the SPREAD is the range (max - min) of the
allpass round medians: the baseline's own run-to-run scatter in this process.  `window_minus_allpass` is to be read against it.

usage: python tools/measure_order_window.py [--reps 30] [--rounds 5] [--out profiles/order_window.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

MODES = ("plain", "window", "allpass")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def set_mode(ctx, s, mode, bands):
    ctx.set_source_order_window(s, 1 if mode == "window" else 0, None)
    ctx.set_source_directivity(s, np.ones((bands, 2), np.float32) if mode == "allpass" else None)


def scene_ctx(pkg, name, bands):
    sc = pkg.scenes.by_name(name, bands)
    ctx = pkg.Context(num_bands=bands)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    return sc, ctx


def sources_around(ctx, sc, n, seed=9):
    rng = np.random.default_rng(seed)
    lo, hi = sc.triangles.min(axis=(0, 1)), sc.triangles.max(axis=(0, 1))
    return [ctx.create_source((np.asarray(sc.source, np.float32) + rng.uniform(-0.03, 0.03, 3).astype(np.float32) * (hi - lo)).astype(np.float32))
            for _ in range(n)]


def summarise(rounds):
    """rounds: {mode: [median of round 0, ...]} in seconds -> medians, the baseline's spread and the difference, in ms"""
    out = {m: round(1e3 * median(v), 4) for m, v in rounds.items()}
    out["round_medians_ms"] = {m: [round(1e3 * x, 4) for x in v] for m, v in rounds.items()}
    out["allpass_spread_ms"] = round(1e3 * (max(rounds["allpass"]) - min(rounds["allpass"])), 4)
    out["window_minus_allpass_ms"] = round(out["window"] - out["allpass"], 4)
    out["window_within_allpass_spread"] = bool(abs(out["window_minus_allpass_ms"]) <= out["allpass_spread_ms"])
    out["window_over_plain"] = round(out["window"] / out["plain"], 4)
    return out


def measure(run, reps, rounds, warm):
    """run(mode, k) does one timed piece of work and returns its seconds; the modes alternate inside every round"""
    for k in range(warm):
        for m in MODES:
            run(m, k)
    res = {m: [] for m in MODES}
    k = warm
    for _ in range(rounds):
        t = {m: [] for m in MODES}
        for _ in range(reps):
            for m in MODES:
                t[m].append(run(m, k))
            k += 1
        for m in MODES:
            res[m].append(median(t[m]))
    return summarise(res)


def cfg3_frame(pkg, reps, rounds):
    sc, ctx = scene_ctx(pkg, "old_mine", 8)
    src = {m: ctx.create_source(sc.source) for m in MODES}
    for m, s in src.items():
        set_mode(ctx, s, m, 8)
    p = pkg.default_params(num_rays=262144, depth=8, seed=1)

    def run(m, k):
        p.seed = 100 + k
        t0 = time.perf_counter()
        ctx.compute_energy_response(src[m], p, want_host=False)
        return time.perf_counter() - t0
    out = measure(run, reps, rounds, 3)
    ctx.close()
    return out


def tick(pkg, name, reps, rounds):
    sc, ctx = scene_ctx(pkg, name, 1)
    src = {m: sources_around(ctx, sc, 32) for m in MODES}
    for m, ss in src.items():
        for s in ss:
            set_mode(ctx, s, m, 1)
    p = pkg.default_params(num_rays=2000, depth=0, seed=1, flags=pkg._capi.FLAG_FIXED_NORM_1000)

    def run(m, k):
        p.seed = 1000 + k
        t0 = time.perf_counter()
        ctx.update_sources(src[m], p)
        return time.perf_counter() - t0
    out = measure(run, reps, rounds, 8)
    ctx.close()
    return out


def stream(pkg, reps, rounds, frames=96):
    sc, ctx = scene_ctx(pkg, "starter_room", 4)
    ctx.set_pipelining(2)
    ctx.set_frames_per_launch(2)
    srcs = sources_around(ctx, sc, 8)
    p = pkg.default_params(num_rays=32768, depth=8, seed=1)
    counters = {}

    def run(m, k):
        set_mode(ctx, srcs[3], m, 4)
        ctx.synchronize()
        c0 = ctx.pipeline_counters()
        t0 = time.perf_counter()
        for i in range(frames):
            p.seed = 10000 * k + i
            ctx.compute_energy_response_async(srcs[i % len(srcs)], p)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / frames
        c1 = ctx.pipeline_counters()   # where the time goes: launches and drains of held frames per stream
        counters[m] = {c: int(c1[c] - c0[c]) for c in ("fused_launches", "flushes", "flushed_frames", "host_waits")}
        return dt
    out = measure(run, reps, rounds, 2)
    ctx.close()
    out["pipeline_counters_per_stream_of_%d_frames" % frames] = counters
    out["note"] = "ms per frame; 8 sources x 32 768 rays, depth 8, starter_room, 4 bands, source 3 of 8 in the mode"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="repetitions per mode and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_window.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    data = {"units": "host wall ms; per mode the median of the round medians; allpass_spread_ms = range of the allpass round medians",
            "reps_per_round": a.reps, "rounds": a.rounds}
    data["cfg3_frame_262144_rays_depth8"] = cfg3_frame(pkg, a.reps, a.rounds)
    print(json.dumps(data["cfg3_frame_262144_rays_depth8"]), flush=True)
    data["tick_32_sources_starter_room"] = tick(pkg, "starter_room", a.reps, a.rounds)
    print(json.dumps(data["tick_32_sources_starter_room"]), flush=True)
    data["pipelined_stream"] = stream(pkg, max(2, a.reps // 6), a.rounds)
    print(json.dumps(data["pipelined_stream"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
