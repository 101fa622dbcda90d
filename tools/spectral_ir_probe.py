#!/usr/bin/env python3
"""FS_FLAG_SPECTRAL_IR against the band-mean reconstruct, alternated in one process:
  - the reference tick (fs_update_sources, 1000 pairs, depth = 0, starter_room) for 1, 8 and 32 sources at B = 8;
  - a one-source synchronous reconstruct at B = 1, 4 and 8;
  - the cfg3 stream (fs_set_pipelining(2), fs_set_frames_per_launch(2), 262 144 rays, depth 8, B = 8) in rays/s;
  - the carrier build (first spectral reconstruct after fs_set_band_edges, less a steady one).
Writes one JSON file (default profiles/spectral_ir_probe.json).  Kernel times: run it under rocprofv3 --kernel-trace --stats.
usage (GPU box): python tools/spectral_ir_probe.py [out.json] [--quick]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402
pkg = graft.load_package()
SPEC = pkg._capi.FLAG_SPECTRAL_IR
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else os.path.join("profiles", "spectral_ir_probe.json")
QUICK = "--quick" in sys.argv
REPS = 3 if QUICK else 7


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def scene_ctx(name, B):
    sc = pkg.scenes.by_name(name, B)
    ctx = pkg.Context(num_bands=B)
    ctx.set_scene(sc.triangles, sc.material_ids, sc.absorption)
    ctx.set_listener(sc.listener)
    return sc, ctx


def tick(out):
    sc, ctx = scene_ctx("starter_room", 8)
    rng = np.random.default_rng(9)
    lo, hi = sc.triangles.min(axis=(0, 1)), sc.triangles.max(axis=(0, 1))
    srcs = [ctx.create_source((np.asarray(sc.source, np.float32) + rng.uniform(-0.03, 0.03, 3).astype(np.float32) * (hi - lo)).astype(np.float32))
            for _ in range(32)]
    res = {}
    for S in (1, 8, 32):
        t = {0: [], SPEC: []}
        for rep in range(REPS):
            for flag in (0, SPEC):                      # alternated
                p = pkg.default_params(num_rays=2000, depth=0, seed=1000 + rep, flags=pkg._capi.FLAG_FIXED_NORM_1000 | flag)
                ts = []
                for i in range(30):
                    p.seed = 1000 + 31 * rep + i
                    t1 = time.perf_counter()
                    ctx.update_sources(srcs[:S], p)
                    ts.append(time.perf_counter() - t1)
                t[flag].append(median(ts[5:]) * 1e3)
        res[str(S)] = {"default_ms": round(median(t[0]), 4), "spectral_ms": round(median(t[SPEC]), 4),
                       "ratio": round(median(t[SPEC]) / median(t[0]), 3), "default_runs": [round(x, 4) for x in t[0]],
                       "spectral_runs": [round(x, 4) for x in t[SPEC]]}
        print("tick", S, res[str(S)], flush=True)
    out["reference_tick_B8"] = res
    ctx.close()


def sync_reconstruct(out):
    res = {}
    for B in (1, 4, 8):
        ctx = pkg.Context(num_bands=B)
        s = ctx.create_source(np.zeros(3, np.float32))
        e = np.zeros((B, ctx.num_bins), np.float32)
        e[:, 2:400] = (0.05 * np.exp(-np.arange(398) / 80.0)).astype(np.float32)
        ctx.update_energy_buffer(s, e)
        ctx.reconstruct_impulse_response(s, pkg.default_params(flags=SPEC))   # (the carriers get built here)
        t = {0: [], SPEC: []}
        for rep in range(REPS):
            for flag in (0, SPEC):
                p = pkg.default_params(flags=flag)
                ts = []
                for _ in range(50):
                    t1 = time.perf_counter()
                    ctx.reconstruct_impulse_response(s, p)
                    ts.append(time.perf_counter() - t1)
                t[flag].append(median(ts[5:]) * 1e3)
        # the carrier build: the first spectral reconstruct after fs_set_band_edges, less a steady one
        builds = []
        for _ in range(3):
            ctx.set_band_edges(None)
            t1 = time.perf_counter()
            ctx.reconstruct_impulse_response(s, pkg.default_params(flags=SPEC))
            builds.append((time.perf_counter() - t1) * 1e3 - median(t[SPEC]))
        res[str(B)] = {"default_ms": round(median(t[0]), 4), "spectral_ms": round(median(t[SPEC]), 4),
                       "ratio": round(median(t[SPEC]) / median(t[0]), 3), "carrier_build_ms_host": round(median(builds), 3)}
        print("reconstruct", B, res[str(B)], flush=True)
        ctx.close()
    out["sync_reconstruct"] = res


def cfg3(out):
    sc, ctx = scene_ctx("starter_room", 8)
    s = ctx.create_source(sc.source)
    ctx.set_pipelining(2)
    ctx.set_frames_per_launch(2)
    rays, steps = 262144, (20 if QUICK else 60)
    r = {0: [], SPEC: []}
    for rep in range(REPS):
        for flag in (0, SPEC):
            p = pkg.default_params(num_rays=rays, depth=8, seed=1, flags=flag)
            for i in range(6):                             # warm-up
                p.seed = 90000 + i
                ctx.compute_energy_response_async(s, p)
                ctx.reconstruct_impulse_response_async(s, p)
            ctx.synchronize()
            t1 = time.perf_counter()
            for i in range(steps):
                p.seed = 1 + i + 1000 * rep
                ctx.compute_energy_response_async(s, p)
                ctx.reconstruct_impulse_response_async(s, p)
            ctx.synchronize()
            r[flag].append(rays * steps / (time.perf_counter() - t1))
    out["cfg3_stream_B8"] = {"default_rays_per_s": round(median(r[0])), "spectral_rays_per_s": round(median(r[SPEC])),
                             "ratio": round(median(r[SPEC]) / median(r[0]), 4),
                             "default_runs": [round(x) for x in r[0]], "spectral_runs": [round(x) for x in r[SPEC]]}
    print("cfg3", out["cfg3_stream_B8"], flush=True)
    ctx.close()


out = {"tool": "tools/spectral_ir_probe.py", "reps_alternated": REPS}
sync_reconstruct(out)
tick(out)
cfg3(out)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
