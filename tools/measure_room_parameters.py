#!/usr/bin/env python3
"""FS_FLAG_ROOM_PARAMETERS: what publishing the room parameters with each impulse response costs, flag off against flag on.

  * fs_update_sources ticks on starter_room (4 bands, 2 000 rays per source, depth 0: the reference's frame) of 1, 32 and 128
    sources — the flagged reconstruct is the same batch launch with count * B more workgroups;
  * the cfg3-style pipelined stream (fs_set_pipelining(2), two frames per launch) of 8 sources x 32 768 rays, depth 8, starter_room,
    every frame followed by its reconstruct — flagged reconstructs leave the fused launch (reconstruct_now / flush_reconstruct).
Host wall time per tick / frame, median over --reps after a warm-up, the two modes alternating in rounds.

--profile-run: 20 ticks of 1, 32 and 128 sources per mode, for `rocprofv3 --kernel-trace --stats` (kernel times);
--merge-trace CSV: fold that run's kernel_trace.csv (reconstruct_batch_kernel with and without the parameter workgroups, by the
  tick's source count, which the grid size gives) into --out.
usage: python tools/measure_room_parameters.py [--reps 30] [--out profiles/room_parameters.json] | --profile-run | --merge-trace CSV"""
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

BANDS = 4
TICKS = (1, 32, 128)


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


def tick(pkg, n, reps):
    sc, ctx = scene_ctx(pkg, "starter_room", BANDS)
    srcs = sources_around(ctx, sc, n)
    flag = pkg._capi.FLAG_ROOM_PARAMETERS
    t = {"off": [], "on": []}
    for r in range(reps + 8):
        for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):   # (the order alternates too)
            p = pkg.default_params(num_rays=2000, depth=0, seed=1000 + r, flags=flag if mode == "on" else 0)
            t0 = time.perf_counter()
            ctx.update_sources(srcs, p)
            if r >= 8:
                t[mode].append(time.perf_counter() - t0)
    ctx.update_sources(srcs, pkg.default_params(num_rays=2000, depth=0, seed=1, flags=flag))   # (a flagged tick last: records to look at)
    seq, rec = ctx.room_parameters(srcs[0])
    assert seq != 0 and np.isfinite(rec["t30"]).any()
    ctx.close()
    out = {k: median_ms(v) for k, v in t.items()}
    out["added_ms"] = round(out["on"] - out["off"], 4)
    out["ratio"] = round(out["on"] / out["off"], 4)
    return out


def stream(pkg, reps, frames=96):
    sc, ctx = scene_ctx(pkg, "starter_room", BANDS)
    ctx.set_pipelining(2)
    ctx.set_frames_per_launch(2)
    srcs = sources_around(ctx, sc, 8)
    flag = pkg._capi.FLAG_ROOM_PARAMETERS
    p = pkg.default_params(num_rays=32768, depth=8, seed=1)
    t = {"off": [], "on": []}
    counters = {}
    for r in range(reps + 2):
        for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):
            rp = pkg.default_params(flags=flag if mode == "on" else 0)
            ctx.synchronize()
            c0 = ctx.pipeline_counters()
            t0 = time.perf_counter()
            for i in range(frames):
                s = srcs[i % len(srcs)]
                p.seed = 10000 * r + i
                ctx.compute_energy_response_async(s, p)
                ctx.reconstruct_impulse_response_async(s, rp)
            ctx.synchronize()
            if r >= 2:
                t[mode].append((time.perf_counter() - t0) / frames)
                c1 = ctx.pipeline_counters()
                counters[mode] = {k: int(c1[k] - c0[k]) for k in ("fused_launches", "flushes", "flushed_frames", "tail_stream_ops",
                                                                   "publishes_by_word", "publishes_by_event")}
    ctx.close()
    out = {k: median_ms(v) for k, v in t.items()}
    out["ratio"] = round(out["on"] / out["off"], 4)
    out["pipeline_counters_per_stream_of_%d_frames" % frames] = counters
    out["note"] = "ms per frame (trace + reconstruct); 8 sources x 32 768 rays, depth 8, starter_room, 4 bands"
    return out


def profile_run(pkg):
    flag = pkg._capi.FLAG_ROOM_PARAMETERS
    for n in TICKS:
        sc, ctx = scene_ctx(pkg, "starter_room", BANDS)
        srcs = sources_around(ctx, sc, n)
        for i in range(20):
            for f in (0, flag):
                ctx.update_sources(srcs, pkg.default_params(num_rays=2000, depth=0, seed=70 + i, flags=f))
        ctx.close()


def merge_trace(path, out):
    """kernel_trace.csv -> per (overload, grid size): calls, median / mean us.  Grid size = count * ((B + 1) * cb [+ B]) workgroups
    of 256 threads: the tick's source count follows (cb = 12 blocks of 4 096 samples for 48 000-sample IRs)."""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "reconstruct_batch_kernel" not in name:
                continue
            grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
            wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256)
            blocks = grid // max(wg, 1)
            room = "float* const*" in name or "float*const*" in name
            per = (BANDS + 1) * 12 + (BANDS if room else 0)
            n = blocks // per if blocks % per == 0 else None
            key = ("with_room_parameters" if room else "plain", n)
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = []
    for (kind, n), us in sorted(rows.items(), key=lambda kv: (str(kv[0][1]), kv[0][0])):
        us = sorted(us)
        res.append({"kernel": "reconstruct_batch_kernel", "workgroups": kind, "sources": n, "calls": len(us),
                    "median_us": round(us[len(us) // 2], 2), "mean_us": round(sum(us) / len(us), 2)})
    data = json.load(open(out)) if os.path.exists(out) else {}
    data["reconstruct_batch_kernel"] = {"source": "rocprofv3 --kernel-trace --stats of --profile-run (20 ticks of 1, 32 and 128 "
                                                  "sources, starter_room, 4 bands, flag off and on alternating)", "rows": res}
    with open(out, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(data["reconstruct_batch_kernel"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "room_parameters.json"))
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
    for n in TICKS:
        data[f"tick_{n}_sources_starter_room"] = tick(pkg, n, a.reps)
        print(n, json.dumps(data[f"tick_{n}_sources_starter_room"]), flush=True)
    data["pipelined_stream"] = stream(pkg, max(4, a.reps // 6))
    print(json.dumps(data["pipelined_stream"]), flush=True)
    data["units"] = "host wall ms, median; ratio = flag on / flag off"
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
