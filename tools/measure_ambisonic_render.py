#!/usr/bin/env python3
"""Ambisonic-voice timing: the median host wall time of one fs_ambisonic_render_process_batch call (1024 stereo frames per source,
8 bands, T = 255, 16 voices per source, every voice's delay, gains and direction ramping in every callback, the copies up and back
and the stream wait included) for {1, 32, 256} sources, orders 0 .. 3 and the three return modes: out only, mix only, both.
Beside it, at the same shapes and in the same session: fs_reflection_render_process_batch and fs_binaural_render_process_batch (a
spherical-head set of 1024 directions, H = 128).  Every (renderer, order) runs in a process of its own, the processes alternate —
reflection, binaural, order 0, 1, 2, 3, and round again — five rounds; a figure is the median over the rounds of the processes'
own medians, with the least and the largest beside it.  The C entry points are called with prepared arrays: the numbers are the
library's, not the Python wrapper's.  Every process also prints a digest of its first out-and-mix callback of 32 sources.
usage: python tools/measure_ambisonic_render.py [reps] [output.json] [rounds]
       python tools/measure_ambisonic_render.py --worker RENDERER ORDER REPS     (one process's medians, as a JSON line)"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME, TAPS, BANDS, VOICES, SOURCES, HRIR_TAPS, DIRECTIONS = 1024, 255, 8, 16, (1, 32, 256), 128, 1024
MODES = ("out", "mix", "both")
RUNS = [("reflection", 0), ("binaural", 0), ("ambisonic", 0), ("ambisonic", 1), ("ambisonic", 2), ("ambisonic", 3)]


def worker(renderer, order, reps):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    cap = pkg._capi
    lib = cap.load()
    rng = np.random.default_rng(0)
    ctx = pkg.Context(num_bands=BANDS)
    channels = (order + 1) ** 2 if renderer == "ambisonic" else 2
    if renderer == "binaural":
        ctx.hrtf_set(*pkg.Context.hrtf_spherical_head(ctx.cfg.sample_rate, DIRECTIONS, HRIR_TAPS))
    srcs = [ctx.create_source() for _ in range(max(SOURCES))]
    for s in srcs:
        if renderer == "reflection":
            ctx.reflection_render_init(s, FRAME, TAPS, VOICES, 0.1)
        elif renderer == "binaural":
            ctx.binaural_render_init(s, FRAME, TAPS, VOICES, 0.1)
        else:
            ctx.ambisonic_render_init(s, FRAME, TAPS, VOICES, 0.1, order)
    call_c = {"reflection": lib.fs_reflection_render_process_batch, "binaural": lib.fs_binaural_render_process_batch,
              "ambisonic": lib.fs_ambisonic_render_process_batch}[renderer]
    dtype = pkg.Context.REFLECTION_VOICE_DTYPE if renderer == "reflection" else pkg.Context.BINAURAL_VOICE_DTYPE
    mono = np.repeat(rng.uniform(-1, 1, (max(SOURCES), FRAME)).astype(np.float32), 2, axis=1)   # a mono source in both channels
    out = np.empty((max(SOURCES), FRAME * channels), np.float32)
    mix = np.empty(FRAME * channels, np.float32)
    result = {"renderer": renderer, "order": order, "channels": channels, "ms": {}, "digest": None}
    for n in SOURCES:
        handles = np.ascontiguousarray(srcs[:n], dtype=np.int32)
        counts = np.full(n, VOICES, np.int32)
        lists = [np.zeros((n, VOICES), dtype=dtype) for _ in range(2)]
        delay = rng.uniform(0.0, 0.05, (n, VOICES))
        for k in range(2):   # the two lists a callback alternates between: every voice continues and ramps everything it has
            lists[k]["key"] = np.arange(VOICES, dtype=np.uint32)[None, :]
            lists[k]["delay"] = delay + 0.004 * k
            lists[k]["band_gain"] = rng.uniform(0.0, 1.0, (n, VOICES, 8))
            if renderer == "reflection":
                lists[k]["channel_gain"] = rng.uniform(-1.0, 1.0, (n, VOICES, 2))
            else:
                lists[k]["gain"] = rng.uniform(-1.0, 1.0, (n, VOICES))
                lists[k]["direction"] = rng.normal(size=(n, VOICES, 3))
        blk = np.ascontiguousarray(mono[:n])
        rows = np.zeros((n, 4), np.uint32)
        flip = [0]
        for mode in MODES:
            def call():
                flip[0] ^= 1
                rc = call_c(ctx.h, handles.ctypes.data, n, blk.ctypes.data, lists[flip[0]].ctypes.data, counts.ctypes.data, VOICES,
                            out.ctypes.data if mode != "mix" else None, mix.ctypes.data if mode != "out" else None, rows.ctypes.data)
                assert rc == cap.OK, rc

            if n == 32 and mode == "both" and result["digest"] is None:   # (the histories are then what the calls before left: the same in every process)
                call()
                result["digest"] = hashlib.sha256(out[:n].tobytes() + mix.tobytes()).hexdigest()[:16]
            for _ in range(10):
                call()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                t.append(1e3 * (time.perf_counter() - t0))
            assert int(rows[:, 0].min()) == VOICES and int(rows[:, 3].max()) == 0
            result["ms"][f"{n}:{mode}"] = float(np.median(t))
    ctx.close()
    print("WORKER " + json.dumps(result), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    per = {run: [] for run in RUNS}
    digests = {run: set() for run in RUNS}
    for rnd in range(rounds):
        for run in RUNS:   # a fresh process each, one at a time
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", run[0], str(run[1]), str(reps)], capture_output=True,
                               text=True, timeout=300, check=True)
            line = [x for x in p.stdout.splitlines() if x.startswith("WORKER ")][-1]
            got = json.loads(line[len("WORKER "):])
            per[run].append(got["ms"])
            digests[run].add(got["digest"])
            print(f"round {rnd} {run[0]} {run[1]}: {got['ms']}", flush=True)

    def stats(run, key):
        v = [m[key] for m in per[run]]
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

    result = {"callback": f"{FRAME} stereo frames per source, {BANDS} bands, T = {TAPS}, {VOICES} voices per source; binaural: H = {HRIR_TAPS}, "
                          f"{DIRECTIONS} directions", "reps": reps, "rounds": rounds, "realtime_budget_ms": FRAME / 48.0, "rows": [],
              "digests": {f"{r[0]}{r[1] if r[0] == 'ambisonic' else ''}": sorted(digests[r]) for r in RUNS}}
    for n in SOURCES:
        for mode in MODES:
            key = f"{n}:{mode}"
            row = {"sources": n, "mode": mode, "reflection_ms": stats(RUNS[0], key), "binaural_ms": stats(RUNS[1], key)}
            for run in RUNS[2:]:
                s = stats(run, key)
                row[f"ambisonic_order{run[1]}_ms"] = s
                row[f"ratio_order{run[1]}_over_reflection"] = s["median"] / row["reflection_ms"]["median"]
            result["rows"].append(row)
    # the share of a call that is the copy back of out (and its copy into the caller's array): 1 - mix only / out only
    result["copy_back_share"] = []
    for n in SOURCES:
        share = {"sources": n, "reflection": 1.0 - stats(RUNS[0], f"{n}:mix")["median"] / stats(RUNS[0], f"{n}:out")["median"]}
        for run in RUNS[2:]:
            share[f"ambisonic_order{run[1]}"] = 1.0 - stats(run, f"{n}:mix")["median"] / stats(run, f"{n}:out")["median"]
        result["copy_back_share"].append(share)
    text = json.dumps(result, indent=1)
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
