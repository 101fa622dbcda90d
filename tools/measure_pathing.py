#!/usr/bin/env python3
"""fs_pathing_bake / fs_update_pathing_paths: what the probe graph costs.

  * host wall time of a bake (median after a warm-up) for N = 256 and 1024 probes on starter_room (4 bands) and old_mine (8 bands);
    the probes are seeded uniform points of the box that holds the scene's sources and listener, grown by 300 cm: no nav mesh
    here, so some stand inside geometry and link to nothing — the edge count and the share of isolated probes are reported;
  * host wall time of an update for 1, 32 and 256 sources (those of tools/measure_reflection2_paths.py), with validate on, and how
    many rows came back FOUND, DIRECT and the largest hops;
  * the Jacobi rounds the listener's relaxation needs, counted by restating it in numpy float32 over the baked graph with the
    listener's attach set taken from fs_trace_rays (no own actors in these scenes).

usage: python tools/measure_pathing.py [--reps 6] [--out profiles/pathing.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft  # noqa: E402
from measure_reflection2_paths import sources  # noqa: E402
from measure_reflection_paths import SCENES, scene_ctx, timed  # noqa: E402

PROBES = (256, 1024)
COUNTS = (1, 32, 256)
WARM = 2
GROW = 300.0


def probes_of(sc, n):
    pts = np.asarray([sc.source, sc.listener] + ([] if sc.extra_sources is None else list(sc.extra_sources)), np.float64)
    lo, hi = pts.min(axis=0) - GROW, pts.max(axis=0) + GROW
    return np.random.default_rng(0xBA4E + n).uniform(lo, hi, (n, 3)).astype(np.float32)


def rounds_of(ctx, pts, graph, listener, max_attach, max_length):
    """Jacobi rounds that change something, d = dL at the start"""
    n = len(pts)
    L = np.asarray(listener, np.float32)
    e = pts - L[None, :]
    a = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    with np.errstate(all="ignore"):
        d = e * (np.float32(1.0) / a)[:, None]
    hit = ctx.trace_rays(np.broadcast_to(L, (n, 3)), np.nan_to_num(d), a, any_hit=False)[0]
    dL = np.where((a <= np.float32(max_attach)) & ~hit, a, np.float32(np.inf)).astype(np.float32)
    adj = ((graph[:, np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)
    ee = pts[None, :, :] - pts[:, None, :]
    w = np.sqrt((ee[..., 0] * ee[..., 0] + ee[..., 1] * ee[..., 1]) + ee[..., 2] * ee[..., 2])
    dist, rounds = dL, 0
    for _ in range(n):
        c = dist[:, None] + w
        new = np.minimum(dist, np.where(adj & (c <= np.float32(max_length)), c, np.float32(np.inf)).min(axis=0))
        if np.array_equal(new.view(np.uint32), dist.view(np.uint32)):
            break
        dist, rounds = new, rounds + 1
    return rounds, int(np.isfinite(dL).sum()), int(np.isfinite(dist).sum())


def grid(pkg, reps):
    out = {}
    defaults = pkg._capi.default_pathing_params()
    for name, bands in SCENES:
        sc, ctx = scene_ctx(pkg, name, bands)
        srcs = sources(ctx, sc, name, max(COUNTS))
        rows = []
        for n in PROBES:
            pts = probes_of(sc, n)
            ctx.pathing_set_probes(pts)
            bake_ms = timed(lambda: ctx.pathing_bake(), reps, warm=WARM)
            edges = ctx.pathing_bake()
            graph = ctx.pathing_graph()
            degree = np.array([sum(bin(int(x)).count("1") for x in r) for r in graph])
            rounds, attached, reached = rounds_of(ctx, pts, graph, sc.listener, defaults.max_attach, defaults.max_length)
            row = {"probes": n, "triangles": int(len(sc.triangles)), "bake_ms": bake_ms, "edges": int(edges), "mean_degree": round(float(degree.mean()), 2),
                   "max_degree": int(degree.max()), "isolated_probes": int((degree == 0).sum()), "listener_attached": attached,
                   "probes_reached": reached, "rounds": rounds, "updates": []}
            for count in COUNTS:
                ms = timed(lambda: ctx.pathing_paths(srcs[:count]), reps, warm=WARM)
                r = ctx.pathing_paths(srcs[:count])
                row["updates"].append({"count": count, "call_ms": ms, "us_per_source": round(1e3 * ms / count, 3),
                                       "found": int(((r["flags"] & 1) != 0).sum()), "direct": int(((r["flags"] & 2) != 0).sum()),
                                       "stale": int(((r["flags"] & 4) != 0).sum()), "max_hops": int(r["hops"].max())})
            print(name, json.dumps(row), flush=True)
            rows.append(row)
        out[name] = rows
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathing.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    data = {"host_wall": grid(pkg, a.reps), "reps": {"timed": a.reps, "warm_up": WARM},
            "units": "host wall ms per call, median after a warm-up; fs_pathing_bake_params and fs_pathing_params at their defaults; "
                     "probes = seeded uniform points of the box round the scene's sources and listener grown by 300 cm"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(data, f, indent=1)


if __name__ == "__main__":
    main()
