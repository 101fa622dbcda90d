#!/usr/bin/env python3
"""fs_update_reflection_paths: what the first-order reflections of a tick cost.

  * host wall time per call (median after a warm-up) for count in {1, 32, 128} on starter_room (4 bands) and old_mine (8 bands),
    sources at the scenes' stock positions (cycled, jittered by a few cm), default parameters; with it the mean candidates and
    reflections found per source and the rows that overflowed;
  * a 32-source fs_update_sources tick (2 000 rays per source, depth 0) with and without a reflection_paths call beside it,
    the two alternating in rounds.

--profile-run: 20 calls per (scene, count) for `rocprofv3 --kernel-trace --stats`; prints the calls made;
--merge-trace KERNEL_CSV: fold that run's trace into --out: reflect_scan_kernel's and reflect_confirm_kernel's times by grid size.
usage: python tools/measure_reflection_paths.py [--reps 30] [--out profiles/reflection_paths.json] | --profile-run | --merge-trace CSV"""
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

SCENES = (("starter_room", 4), ("old_mine", 8))
COUNTS = (1, 32, 128)
PROFILE_CALLS = 20
KERNELS = ("reflect_scan_kernel", "reflect_confirm_kernel")


def median_ms(xs):
    xs = sorted(xs)
    return round(1e3 * xs[len(xs) // 2], 4)


def scene_ctx(pkg, name, bands):
    sc = pkg.scenes.by_name(name, bands)
    tr, sca = pkg.scenes.material_lobes(sc)
    ctx = pkg.Context(num_bands=bands)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption, tr, sca, object_ids=sc.object_ids)
    ctx.set_listener(sc.listener)
    return sc, ctx


def stock_sources(ctx, sc, n, seed=9):
    stock = [np.asarray(sc.source, np.float32)] + ([np.asarray(p, np.float32) for p in sc.extra_sources] if sc.extra_sources is not None else [])
    rng = np.random.default_rng(seed)
    return [ctx.create_source((stock[i % len(stock)] + (rng.uniform(-5.0, 5.0, 3) if i >= len(stock) else 0.0)).astype(np.float32))
            for i in range(n)]


def timed(fn, reps, warm=5):
    t = []
    for r in range(reps + warm):
        t0 = time.perf_counter()
        fn()
        if r >= warm:
            t.append(time.perf_counter() - t0)
    return median_ms(t)


def grid(pkg, reps):
    out = {}
    for name, bands in SCENES:
        sc, ctx = scene_ctx(pkg, name, bands)
        srcs = stock_sources(ctx, sc, max(COUNTS))
        rows = []
        for count in COUNTS:
            ms = timed(lambda: ctx.reflection_paths(srcs[:count]), reps)
            r, _ = ctx.reflection_paths(srcs[:count])
            rows.append({"count": count, "triangles": int(len(sc.triangles)), "call_ms": ms, "us_per_source": round(1e3 * ms / count, 3),
                         "mean_candidates": round(float(r["candidates"].mean()), 2), "mean_found": round(float(r["found"].mean()), 2),
                         "rows_overflowed": int((r["flags"] != 0).sum())})
            print(name, json.dumps(rows[-1]), flush=True)
        out[name] = rows
        ctx.close()
    return out


def tick_beside(pkg, reps):
    sc, ctx = scene_ctx(pkg, "starter_room", 4)
    srcs = stock_sources(ctx, sc, 32)
    t = {"tick": [], "tick_and_reflection_paths": []}
    for r in range(reps + 8):
        for mode in (("tick", "tick_and_reflection_paths") if r % 2 == 0 else ("tick_and_reflection_paths", "tick")):   # (the order alternates too)
            p = pkg.default_params(num_rays=2000, depth=0, seed=1000 + r)
            t0 = time.perf_counter()
            ctx.update_sources(srcs, p)
            if mode != "tick":
                ctx.reflection_paths(srcs)
            if r >= 8:
                t[mode].append(time.perf_counter() - t0)
    ctx.close()
    out = {k: median_ms(v) for k, v in t.items()}
    out["added_ms"] = round(out["tick_and_reflection_paths"] - out["tick"], 4)
    out["note"] = "32 sources, starter_room, 4 bands, 2 000 rays per source, depth 0; reflection_paths with the default parameters"
    return out


def profile_run(pkg):
    calls = 0
    for name, bands in SCENES:
        sc, ctx = scene_ctx(pkg, name, bands)
        srcs = stock_sources(ctx, sc, max(COUNTS))
        for count in COUNTS:
            for _ in range(PROFILE_CALLS):
                ctx.reflection_paths(srcs[:count])
                calls += 1
        ctx.close()
    print(json.dumps({"reflection_paths_calls": calls, "contexts": len(SCENES)}), flush=True)


def merge_trace(path, out):
    """kernel_trace.csv -> the two kernels by grid size (workgroups of 256 threads: 256 triangles of the scan, 4 rows of the
    confirmation): dispatches, median / mean / max us"""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            k = next((k for k in KERNELS if k in r.get("Kernel_Name", "")), None)
            if k is None:
                continue
            g = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
            wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256)
            rows.setdefault((k, g // max(wg, 1)), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = []
    for (k, blocks), us in sorted(rows.items()):
        us = sorted(us)
        res.append({"kernel": k, "workgroups": blocks, "dispatches": len(us), "median_us": round(us[len(us) // 2], 2),
                    "mean_us": round(sum(us) / len(us), 2), "max_us": round(us[-1], 2)})
    data = json.load(open(out)) if os.path.exists(out) else {}
    data["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of --profile-run (%d calls per scene and count; the scan's grid is the "
                                      "scene's, whatever count is: its rows mix the counts)" % PROFILE_CALLS,
                            "reflection_paths_calls": len(SCENES) * len(COUNTS) * PROFILE_CALLS, "rows": res}
    with open(out, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(data["kernel_trace"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reflection_paths.json"))
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--merge-trace")
    a = ap.parse_args()
    if a.merge_trace is not None:
        if not os.path.exists(a.merge_trace):
            sys.exit(f"no kernel trace file: {a.merge_trace!r}")
        merge_trace(a.merge_trace, a.out)
        return
    pkg = graft.load_package()
    if a.profile_run:
        profile_run(pkg)
        return
    data = json.load(open(a.out)) if os.path.exists(a.out) else {}
    data["host_wall"] = grid(pkg, a.reps)
    data["tick_32_sources_starter_room"] = tick_beside(pkg, a.reps)
    print(json.dumps(data["tick_32_sources_starter_room"]), flush=True)
    data["units"] = "host wall ms per call, median after a warm-up; default fs_reflection_params"
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
