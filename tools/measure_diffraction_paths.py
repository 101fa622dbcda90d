#!/usr/bin/env python3
"""fs_update_diffraction_paths: what the first-order edge diffraction of a tick costs.

  * host wall time per call (median after a warm-up) for count in {1, 32, 128} on starter_room (4 bands) and old_mine (8 bands),
    sources at the scenes' stock positions (cycled, jittered by a few cm), default parameters; with it the mean candidates,
    confirmed and found per source and the rows that overflowed;
  * fs_update_reflection_paths at the same counts with the same sources in the same process, beside it;
  * a 32-source fs_update_sources tick (2 000 rays per source, depth 0) with and without a diffraction_paths call beside it,
    the two alternating in rounds.

usage: python tools/measure_diffraction_paths.py [--reps 30] [--out profiles/diffraction_paths.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from measure_reflection_paths import COUNTS, SCENES, median_ms, scene_ctx, stock_sources, timed  # noqa: E402


def grid(pkg, reps):
    out = {}
    for name, bands in SCENES:
        sc, ctx = scene_ctx(pkg, name, bands)
        srcs = stock_sources(ctx, sc, max(COUNTS))
        rows = []
        for count in COUNTS:
            ms = timed(lambda: ctx.diffraction_paths(srcs[:count]), reps)
            refl = timed(lambda: ctx.reflection_paths(srcs[:count]), reps)
            r, _ = ctx.diffraction_paths(srcs[:count])
            rows.append({"count": count, "triangles": int(len(sc.triangles)), "call_ms": ms, "us_per_source": round(1e3 * ms / count, 3),
                         "reflection_paths_call_ms": refl,
                         "mean_candidates": round(float(r["candidates"].mean()), 2), "mean_confirmed": round(float(r["confirmed"].mean()), 2),
                         "mean_found": round(float(r["found"].mean()), 2), "rows_overflowed": int((r["flags"] != 0).sum())})
            print(name, json.dumps(rows[-1]), flush=True)
        out[name] = rows
        ctx.close()
    return out


def tick_beside(pkg, reps):
    import time
    sc, ctx = scene_ctx(pkg, "starter_room", 4)
    srcs = stock_sources(ctx, sc, 32)
    t = {"tick": [], "tick_and_diffraction_paths": []}
    for r in range(reps + 8):
        for mode in (("tick", "tick_and_diffraction_paths") if r % 2 == 0 else ("tick_and_diffraction_paths", "tick")):   # (the order alternates too)
            p = pkg.default_params(num_rays=2000, depth=0, seed=1000 + r)
            t0 = time.perf_counter()
            ctx.update_sources(srcs, p)
            if mode != "tick":
                ctx.diffraction_paths(srcs)
            if r >= 8:
                t[mode].append(time.perf_counter() - t0)
    ctx.close()
    out = {k: median_ms(v) for k, v in t.items()}
    out["added_ms"] = round(out["tick_and_diffraction_paths"] - out["tick"], 4)
    out["note"] = "32 sources, starter_room, 4 bands, 2 000 rays per source, depth 0; diffraction_paths with the default parameters"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffraction_paths.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    data = json.load(open(a.out)) if os.path.exists(a.out) else {}
    data["host_wall"] = grid(pkg, a.reps)
    data["tick_32_sources_starter_room"] = tick_beside(pkg, a.reps)
    print(json.dumps(data["tick_32_sources_starter_room"]), flush=True)
    data["units"] = "host wall ms per call, median after a warm-up; default fs_diffraction_params and fs_reflection_params"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
