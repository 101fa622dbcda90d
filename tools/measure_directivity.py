#!/usr/bin/env python3
"""Source directivity (fs_source_set_directivity): what a directional source costs, against the same work omnidirectional.

  * a waited-for cfg3 frame: old_mine, 8 bands, 262 144 rays, depth 8 (fs_compute_energy_response);
  * a tick of 32 sources (fs_update_sources: 2 000 rays each, depth 0, the reference's frame) on starter_room and old_mine,
    every source directional;
  * a pipelined stream (fs_set_pipelining(2), two frames per launch) of 8 sources x 32 768 rays, depth 8, starter_room, in
    which one source is directional — its frames are not held, so they end the fused launches around them.
Host wall time per frame / tick, median over --reps after a warm-up, the two modes alternating in rounds.

--profile-run: only a short mix of the frames above, for `rocprofv3 --kernel-trace --stats` (kernel times);
--merge-stats CSV: fold that run's kernel_stats.csv (the connect kernels) into --out.
usage: python tools/measure_directivity.py [--reps 30] [--out profiles/directivity.json] | --profile-run | --merge-stats CSV"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

OBLIQUE = (0.3, -0.8, 0.52)


def cardioid(bands, K=181):
    th = np.arange(K) * np.pi / (K - 1)
    return np.stack([(0.5 * (1.0 + np.cos(th))) ** (1 + 1.5 * b) + 0.02 for b in range(bands)]).astype(np.float32)


def median_ms(xs):
    xs = sorted(xs)
    return round(1e3 * xs[len(xs) // 2], 4)


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


def cfg3_frame(pkg, reps):
    sc, ctx = scene_ctx(pkg, "old_mine", 8)
    omni, dirs = ctx.create_source(sc.source), ctx.create_source(sc.source)
    ctx.set_source_orientation(dirs, OBLIQUE)
    ctx.set_source_directivity(dirs, cardioid(8))
    p = pkg.default_params(num_rays=262144, depth=8, seed=1)
    t = {"omni": [], "directional": []}
    for r in range(reps + 3):
        for mode, s in (("omni", omni), ("directional", dirs)):
            p.seed = 100 + r
            t0 = time.perf_counter()
            ctx.compute_energy_response(s, p, want_host=False)
            if r >= 3:
                t[mode].append(time.perf_counter() - t0)
    ctx.close()
    out = {k: median_ms(v) for k, v in t.items()}
    out["ratio"] = round(out["directional"] / out["omni"], 4)
    return out


def tick(pkg, name, reps):
    sc, ctx = scene_ctx(pkg, name, 1)
    omni, dirs = sources_around(ctx, sc, 32), sources_around(ctx, sc, 32)
    for s in dirs:
        ctx.set_source_orientation(s, OBLIQUE)
        ctx.set_source_directivity(s, cardioid(1))
    p = pkg.default_params(num_rays=2000, depth=0, seed=1, flags=pkg._capi.FLAG_FIXED_NORM_1000)
    t = {"omni": [], "directional": []}
    for r in range(reps + 8):
        for mode, ss in (("omni", omni), ("directional", dirs)):
            p.seed = 1000 + r
            t0 = time.perf_counter()
            ctx.update_sources(ss, p)
            if r >= 8:
                t[mode].append(time.perf_counter() - t0)
    ctx.close()
    out = {k: median_ms(v) for k, v in t.items()}
    out["ratio"] = round(out["directional"] / out["omni"], 4)
    return out


def stream(pkg, reps, frames=96):
    sc, ctx = scene_ctx(pkg, "starter_room", 4)
    ctx.set_pipelining(2)
    ctx.set_frames_per_launch(2)
    srcs = sources_around(ctx, sc, 8)
    p = pkg.default_params(num_rays=32768, depth=8, seed=1)
    t = {"omni": [], "one_directional": []}
    counters = {}
    for r in range(reps + 2):
        for mode in ("omni", "one_directional"):
            ctx.set_source_directivity(srcs[3], cardioid(4) if mode == "one_directional" else None)
            ctx.synchronize()
            c0 = ctx.pipeline_counters()
            t0 = time.perf_counter()
            for i in range(frames):
                s = srcs[i % len(srcs)]
                ctx.set_source_orientation(s, (np.cos(0.1 * i), np.sin(0.1 * i), 0.2))
                p.seed = 10000 * r + i
                ctx.compute_energy_response_async(s, p)
            ctx.synchronize()
            if r >= 2:
                t[mode].append((time.perf_counter() - t0) / frames)
                c1 = ctx.pipeline_counters()   # where the time goes: launches and drains of held frames per stream
                counters[mode] = {k: int(c1[k] - c0[k]) for k in ("fused_launches", "flushes", "flushed_frames", "host_waits")}
    ctx.close()
    out = {k: median_ms(v) for k, v in t.items()}
    out["ratio"] = round(out["one_directional"] / out["omni"], 4)
    out["pipeline_counters_per_stream_of_%d_frames" % frames] = counters
    out["note"] = "ms per frame; 8 sources x 32 768 rays, depth 8, starter_room, 4 bands, source 3 of 8 directional in the second mode"
    return out


def profile_run(pkg):
    sc, ctx = scene_ctx(pkg, "old_mine", 8)
    a, b = ctx.create_source(sc.source), ctx.create_source(sc.source)
    ctx.set_source_orientation(b, OBLIQUE)
    ctx.set_source_directivity(b, cardioid(8))
    p = pkg.default_params(num_rays=262144, depth=8, seed=1)
    for i in range(10):
        p.seed = 50 + i
        ctx.compute_energy_response(a, p, want_host=False)
        ctx.compute_energy_response(b, p, want_host=False)
    ctx.close()
    for name in ("starter_room", "old_mine"):
        sc, ctx = scene_ctx(pkg, name, 1)
        omni, dirs = sources_around(ctx, sc, 32), sources_around(ctx, sc, 32)
        for s in dirs:
            ctx.set_source_directivity(s, cardioid(1))
        p = pkg.default_params(num_rays=2000, depth=0, seed=1, flags=pkg._capi.FLAG_FIXED_NORM_1000)
        for i in range(20):
            p.seed = 70 + i
            ctx.update_sources(omni, p)
            ctx.update_sources(dirs, p)
        ctx.close()


def merge_stats(path, out):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "connect" in r["Name"]:
                name = r["Name"].split("(anonymous namespace)::")[-1]
                rows.append({"kernel": name[:name.index(">(") + 1] if ">(" in name else name, "calls": int(r["Calls"]),
                             "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                             "max_us": round(float(r["MaxNs"]) / 1e3, 2)})
    data = json.load(open(out)) if os.path.exists(out) else {}
    data["connect_kernels"] = {"source": "rocprofv3 --kernel-trace --stats of --profile-run (10 cfg3 frames and 20 ticks of "
                                         "32 sources per scene, omni and directional alternating)", "rows": rows}
    with open(out, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(data["connect_kernels"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "directivity.json"))
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--merge-stats")
    a = ap.parse_args()
    if a.merge_stats is not None:
        if not os.path.exists(a.merge_stats):
            sys.exit(f"no kernel stats file: {a.merge_stats!r}")
        merge_stats(a.merge_stats, a.out)
        return
    pkg = graft.load_package()
    if a.profile_run:
        profile_run(pkg)
        return
    data = json.load(open(a.out)) if os.path.exists(a.out) else {}
    data["cfg3_frame_262144_rays_depth8"] = cfg3_frame(pkg, a.reps)
    print(json.dumps(data["cfg3_frame_262144_rays_depth8"]), flush=True)
    for name in ("starter_room", "old_mine"):
        data[f"tick_32_sources_{name}"] = tick(pkg, name, a.reps)
        print(name, json.dumps(data[f"tick_32_sources_{name}"]), flush=True)
    data["pipelined_stream"] = stream(pkg, max(4, a.reps // 6))
    print(json.dumps(data["pipelined_stream"]), flush=True)
    data["units"] = "host wall ms, median; ratio = directional / omni"
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
