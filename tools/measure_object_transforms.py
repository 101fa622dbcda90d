#!/usr/bin/env python3
"""Movers per tick at cfg3 (old_mine, 100 000 triangles cut into props): host wall time around "move, then one waited-for
fs_compute_energy_response of 16 384 rays", by two routes alternated tick by tick in one process —
  (a) numpy transform of the movers' vertices, then one fs_scene_update_triangles per mover (36 B per triangle, a wait each);
  (b) one fs_scene_set_object_transforms (48 B per mover, no wait) —
for one mover of 2 000 triangles and for 16 movers of 500 triangles each.  Product path only; fails without a GPU.
Under `rocprofv3 --kernel-trace --stats` the same run gives transform_objects_kernel against the update_tris_kernel launches.
usage: python tools/measure_object_transforms.py [--ticks 60] [--out profiles/object_transforms.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ticks", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.ticks >= 50

pkg = graft.load_package()
sc = pkg.scenes.old_mine(8)
T = sc.triangles.shape[0]
rest = np.ascontiguousarray(sc.triangles, np.float32).reshape(T, 3, 3)


def matrix(tick, k):
    """a small rigid motion about the z axis, different every tick and for every mover"""
    a = 0.002 * ((tick % 7) + 1) + 0.0005 * k
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0, 0.5 * (tick % 5)], [s, c, 0, -0.25 * k], [0, 0, 1, 0.125 * (tick % 3)]], np.float32)


def xf(m, p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], axis=-1)


def run(label, movers, size):
    """props of `size` triangles each (contiguous, as a shim registers components); the first `movers` of them move"""
    obj = (np.arange(T) // size).astype(np.uint32)
    ctx = pkg.Context(num_bands=8)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption, object_ids=obj)
    ctx.set_listener(sc.listener)
    src = ctx.create_source(sc.source)
    prm = pkg.default_params(num_rays=16384, depth=8)
    ids = np.arange(movers, dtype=np.uint32) + 3                   # props 3 .. 3 + movers - 1
    times = {"update_triangles": [], "set_object_transforms": []}
    for tick in range(2 * (args.warmup + args.ticks)):
        route = "update_triangles" if tick % 2 == 0 else "set_object_transforms"
        mats = np.stack([matrix(tick, k) for k in range(movers)])
        prm.seed = tick
        t0 = time.perf_counter()
        if route == "update_triangles":
            for k, i in enumerate(ids):
                first = int(i) * size
                ctx.update_triangles(first, xf(mats[k], rest[first:first + size]))
        else:
            ctx.set_object_transforms(ids, mats)
        ctx.compute_energy_response(src, prm, want_host=False)
        dt = 1e3 * (time.perf_counter() - t0)
        if tick >= 2 * args.warmup:
            times[route].append(dt)
    ctx.close()
    out = {"movers": movers, "triangles_per_mover": size, "ticks_per_route": args.ticks}
    for route, v in times.items():
        v = np.asarray(v)
        out[route] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)),
                      "min_ms": float(v.min()), "max_ms": float(v.max())}
    out["speedup_median"] = out["update_triangles"]["median_ms"] / out["set_object_transforms"]["median_ms"]
    print(label, json.dumps(out), flush=True)
    return out


res = {"scene": "old_mine 100000 triangles, 16384 rays, depth 8, 8 bands",
       "tick": "move, then one waited-for fs_compute_energy_response; host wall time, routes alternated tick by tick",
       "one mover of 2000": run("1 x 2000", 1, 2000), "16 movers of 500": run("16 x 500", 16, 500)}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
