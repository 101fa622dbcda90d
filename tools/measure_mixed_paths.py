#!/usr/bin/env python3
"""fs_update_mixed_paths: what the paths off one reflector and round one edge of a tick cost.

  * host wall time per call (median after a warm-up) for count in {1, 32, 128} and max_length in {500, 750, 1000, 1500} cm on
    starter_room (4 bands, sources at the scene's stock positions, cycled and jittered by a few cm) and old_mine (8 bands, sources
    drawn within 600 cm of the listener: those of tools/measure_reflection2_paths.py and tools/measure_diffraction2_paths.py);
    max_near and max_candidates at their caps so that the counts are seen whole; with it the mean near, candidates, confirmed and
    found per source and the rows that overflow the caps and would overflow the defaults — the sweep the default max_length is
    chosen by;
  * fs_update_diffraction_paths and fs_update_reflection2_paths, both at their defaults, at the same counts with the same sources
    in the same process, beside it.

--profile-run: PROFILE_CALLS calls per (scene, max_length, count), in the order of the grid, for `rocprofv3 --kernel-trace --stats`;
--merge-trace KERNEL_CSV: fold that run's trace into --out: the three kernels' times per (scene, max_length, count) — the i-th
  dispatch of a kernel belongs to the i-th call.
usage: python tools/measure_mixed_paths.py [--reps 6] [--out profiles/mixed_paths.json] | --profile-run | --merge-trace CSV"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from measure_reflection2_paths import sources  # noqa: E402
from measure_reflection_paths import COUNTS, SCENES, scene_ctx, timed  # noqa: E402

LENGTHS = (500.0, 750.0, 1000.0, 1500.0)
PROFILE_CALLS = 4
WARM = 2
KERNELS = ("mixed_near_kernel", "mixed_pair_kernel", "mixed_confirm_kernel")
CAPS = dict(max_near=32768, max_candidates=2048)


def plan():
    return [(name, bands, length, count) for name, bands in SCENES for length in LENGTHS for count in COUNTS]


def grid(pkg, reps):
    out, defaults = {}, pkg._capi.default_mixed_params()
    for name, bands in SCENES:
        sc, ctx = scene_ctx(pkg, name, bands)
        srcs = sources(ctx, sc, name, max(COUNTS))
        rows = []
        for length in LENGTHS:
            for count in COUNTS:
                ms = timed(lambda: ctx.mixed_paths(srcs[:count], max_length=length, **CAPS), reps, warm=WARM)
                first = timed(lambda: ctx.diffraction_paths(srcs[:count]), reps, warm=WARM)
                refl2 = timed(lambda: ctx.reflection2_paths(srcs[:count]), reps, warm=WARM)
                r, _ = ctx.mixed_paths(srcs[:count], max_length=length, **CAPS)
                rows.append({"count": count, "max_length": length, "triangles": int(len(sc.triangles)), "call_ms": ms,
                             "us_per_source": round(1e3 * ms / count, 3), "diffraction_paths_call_ms": first,
                             "reflection2_paths_call_ms": refl2,
                             "mean_near": round(float(r["near"].mean()), 1), "max_near": int(r["near"].max()),
                             "mean_candidates": round(float(r["candidates"].mean()), 2),
                             "mean_confirmed": round(float(r["confirmed"].mean()), 2), "mean_found": round(float(r["found"].mean()), 2),
                             "rows_overflowed": int((r["flags"] != 0).sum()),
                             "rows_beyond_default_max_near": int((r["near"] > defaults.max_near).sum()),
                             "rows_beyond_default_max_candidates": int((r["candidates"] > defaults.max_candidates).sum())})
                print(name, json.dumps(rows[-1]), flush=True)
        out[name] = rows
        ctx.close()
    return out


def profile_run(pkg):
    calls = 0
    for name, bands in SCENES:
        sc, ctx = scene_ctx(pkg, name, bands)
        srcs = sources(ctx, sc, name, max(COUNTS))
        for length in LENGTHS:
            for count in COUNTS:
                for _ in range(PROFILE_CALLS):
                    ctx.mixed_paths(srcs[:count], max_length=length, **CAPS)
                    calls += 1
        ctx.close()
    print(json.dumps({"mixed_paths_calls": calls, "contexts": len(SCENES)}), flush=True)


def merge_trace(path, out):
    """kernel_trace.csv -> per (scene, max_length, count) the three kernels' median us over the configuration's PROFILE_CALLS calls"""
    spans = {k: [] for k in KERNELS}
    with open(path) as f:
        for r in csv.DictReader(f):
            k = next((k for k in KERNELS if k in r.get("Kernel_Name", "")), None)
            if k is not None:
                spans[k].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    configs, res = plan(), []
    for k in KERNELS:
        spans[k].sort()
        if len(spans[k]) != len(configs) * PROFILE_CALLS:
            sys.exit(f"{k}: {len(spans[k])} dispatches in the trace, {len(configs) * PROFILE_CALLS} calls in the plan")
    for i, (name, _, length, count) in enumerate(configs):
        row = {"scene": name, "max_length": length, "count": count}
        for k in KERNELS:
            us = sorted(u for _, u in spans[k][i * PROFILE_CALLS:(i + 1) * PROFILE_CALLS])
            row[k + "_median_us"] = round(us[len(us) // 2], 2)
        res.append(row)
    data = json.load(open(out)) if os.path.exists(out) else {}
    data["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of --profile-run (%d calls per scene, max_length and count)" % PROFILE_CALLS,
                            "rows": res}
    with open(out, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(data["kernel_trace"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_paths.json"))
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
    data["reps"] = {"timed": a.reps, "warm_up": WARM}
    data["units"] = ("host wall ms per call, median after a warm-up; fs_mixed_params at their defaults but for max_length and "
                     "max_near = 32768, max_candidates = 2048; fs_diffraction_params and fs_reflection2_params at their defaults")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
