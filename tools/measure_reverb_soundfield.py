#!/usr/bin/env python3
"""Soundfield late reverb (fs_reverb_soundfield_process_batch): host wall time of one call that serves S soundfield sources, at
orders 0 to 3, against one fs_reverb_process_batch for S mono partitioned sources of the same build.

  * 1024 stereo frames, 48 000 samples, 8 bands; S in {1, 32, 128}; orders 0 .. 3 (C = 1, 4, 9, 16 channels, P = 1, 2, 5, 8 pairs);
    `mix` only and `out` only; two variants: a take in every callback (a new installed IR before each, no crossfade) and no
    take (a constant IR).  The mono rows return `out` (their row is one stereo row whatever the mode);
  * the series alternate, one process per series and repeat; reported are the medians over all repeats with min and max, the
    ratio to the mono rows, and the bytes of spectra the product reads per source (P K N float2 of G and K N of X);
  * no ratio is fixed in advance.  The prediction to confront: the time follows the P spectrum streams the product reads,
    about 6 MB per source per callback at order 3 — and with `out` the copy back of S F C floats takes over at some size;
  * with --parent-lib every series also runs against a library built from the PARENT commit, alternating with this build's: a row
    passes when the median of this build's per-process medians lies within the min - max of the parent's (DESIGN.md section 8's
    rule), and the sha256 digests of the timed outputs are equal.

usage: python tools/measure_reverb_soundfield.py [--parent-lib PATH] [--callbacks 200] [--repeats 5] [--out profiles/reverb_soundfield.json]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_reverb_batch as mb  # noqa: E402
from measure_reverb_ears import BANDS, FRAME, PARTITIONED, SIZES, Lib  # noqa: E402

VARIANTS = ("take_every_callback", "no_take")
MODES = ("mix", "out")
ORDERS = (0, 1, 2, 3)


def bind(lib):
    vp, i32 = C.c_void_p, C.c_int32
    for name, args in (("fs_reverb_soundfield_set", [vp, i32]), ("fs_reverb_set_soundfield", [vp, i32, i32]),
                       ("fs_reverb_soundfield_process_batch", [vp, vp, i32, vp, vp, C.c_uint32, vp])):
        getattr(lib.lib, name).argtypes = args
        getattr(lib.lib, name).restype = C.c_int


def series_times(lib, order, callbacks, warmup):
    """{S: {variant: {mode: {"times": [seconds per callback], "sha256": of the timed outputs}}}}; order < 0: the mono partitioned
    rows (mode "out" only); same seeded inputs and IRs whatever the series"""
    rng = np.random.default_rng(0)
    irs = [mb.noise_ir(rng, lib.n) for _ in range(4)]
    field = order >= 0
    channels = (order + 1) ** 2 if field else 2
    if field:
        bind(lib)
        lib.ok(lib.lib.fs_reverb_soundfield_set(lib.h, order))
    pools = {}
    for v in VARIANTS:
        pool = [lib.source() for _ in range(max(SIZES))]
        for s in pool:
            lib.ok(lib.lib.fs_reverb_set_engine(lib.h, s, PARTITIONED))
            if field:
                lib.ok(lib.lib.fs_reverb_set_soundfield(lib.h, s, 1))
            lib.ok(lib.lib.fs_reverb_init(lib.h, s, FRAME))
            lib.ok(lib.lib.fs_set_impulse_response(lib.h, s, irs[0].ctypes.data, lib.n))
        pools[v] = pool
    res = {}
    for S in SIZES:
        blk = np.clip(rng.normal(0, 0.3, (S, 2 * FRAME)), -1, 1).astype(np.float32)
        out = np.empty((S, FRAME * channels), np.float32)
        mix = np.empty(FRAME * channels, np.float32)
        for v in VARIANTS:
            srcs = np.array(pools[v][:S], np.int32)
            for mode in MODES if field else ("out",):
                o = out.ctypes.data if mode == "out" else None
                m = mix.ctypes.data if mode == "mix" else None

                def call():
                    t = time.perf_counter()
                    if field:
                        rc = lib.lib.fs_reverb_soundfield_process_batch(lib.h, srcs.ctypes.data, S, blk.ctypes.data, o, 0, m)
                    else:
                        rc = lib.lib.fs_reverb_process_batch(lib.h, srcs.ctypes.data, S, blk.ctypes.data, o, None, 0, None)
                    dt = time.perf_counter() - t
                    lib.ok(rc)
                    return dt

                times, sha = [], hashlib.sha256()
                for i in range(warmup + callbacks):
                    if v == "take_every_callback":
                        for s in srcs:
                            lib.ok(lib.lib.fs_set_impulse_response(lib.h, int(s), irs[i % 4].ctypes.data, lib.n))
                    dt = call()
                    if i >= warmup:
                        times.append(dt)
                        sha.update((out if mode == "out" else mix).tobytes())
                res.setdefault(str(S), {}).setdefault(v, {})[mode] = {"times": times, "sha256": sha.hexdigest()}
    return res


def stats(per_process):
    """mb.stats over all repeats, with the min and max and the per-process medians"""
    ts = np.concatenate(per_process)
    st = mb.stats(ts)
    st["min_ms"], st["max_ms"] = float(ts.min()) * 1e3, float(ts.max()) * 1e3
    st["process_medians_ms"] = [float(np.median(t)) * 1e3 for t in per_process]
    return st


def run_worker(path, order, callbacks, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", path, "--order", str(order), "--callbacks", str(callbacks),
           "--warmup", str(warmup)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if p.returncode or not line:
        sys.exit(f"{cmd} failed with status {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libfrequensee.so built from the parent commit: every series against it too")
    ap.add_argument("--callbacks", type=int, default=200, help="timed callbacks per process, size, variant and mode")
    ap.add_argument("--repeats", type=int, default=5, help="processes per series")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--order", type=int, default=-1, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    capi = mb.graft.load_package()._capi
    if a.worker:
        lib = Lib(a.lib, capi)
        res = series_times(lib, a.order, a.callbacks, a.warmup)
        lib.close()
        print("RESULT " + json.dumps(res))
        return 0
    if a.parent_lib and not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: no such file")
    series = (-1,) + ORDERS
    raw = {o: {} for o in series}      # [order][S][variant][mode] -> list of per-process time lists
    praw = {o: {} for o in series}     # the same of the parent's library
    bits, pbits = {}, {}               # [(order, S, variant, mode)] -> the set of digests
    for r in range(a.repeats):
        for o in series:
            for path, into, digests in ((a.parent_lib, praw, pbits), (capi.LIB_PATH, raw, bits)):
                if not path:
                    continue
                for S, vs in run_worker(path, o, a.callbacks, a.warmup).items():
                    for v, ms in vs.items():
                        for mode, got in ms.items():
                            into[o].setdefault(S, {}).setdefault(v, {}).setdefault(mode, []).append(got["times"])
                            digests.setdefault((o, S, v, mode), set()).add(got["sha256"])
            print(f"repeat {r} order {o} done", file=sys.stderr, flush=True)
    n = 1
    while n < 2 * FRAME:
        n *= 2
    K = -(-48000 // FRAME)
    rec = {"callback": f"one fs_reverb_soundfield_process_batch, {FRAME} stereo frames, 48000 samples, {BANDS} bands; mono = one "
                       "fs_reverb_process_batch of partitioned rows returning out",
           "repeats": a.repeats, "callbacks_per_process": a.callbacks, "rows": {}}
    within = total = 0

    def against_parent(st, o, S, v, mode):
        """the parent's repeats of the same series beside this build's: the house rule and the digests"""
        nonlocal within, total
        if not a.parent_lib:
            return
        pm = [float(np.median(t)) * 1e3 for t in praw[o][str(S)][v][mode]]
        med = float(np.median(st["process_medians_ms"]))
        st["parent_process_medians_ms"] = pm
        st["median_of_medians_ms"] = med
        st["within_parent_min_max"] = bool(min(pm) <= med <= max(pm))
        st["over_parent"] = med / float(np.median(pm))
        key = (o, str(S), v, mode)
        st["sha256"] = sorted(bits[key])
        st["bits_equal_parent"] = bits[key] == pbits[key] and len(bits[key]) == 1
        within += st["within_parent_min_max"]
        total += 1

    for S in SIZES:
        row = {}
        for v in VARIANTS:
            mono = stats(raw[-1][str(S)][v]["out"])
            against_parent(mono, -1, S, v, "out")
            e = {"mono": mono}
            for o in ORDERS:
                P = ((o + 1) ** 2 + 1) // 2
                entry = {"channels": (o + 1) ** 2, "pairs": P, "product_reads_bytes_per_source": 8 * n * K * (P + 1),
                         "out_bytes": 4 * S * FRAME * (o + 1) ** 2}
                for mode in MODES:
                    st = stats(raw[o][str(S)][v][mode])
                    st["over_mono"] = st["median_ms"] / mono["median_ms"]
                    against_parent(st, o, S, v, mode)
                    entry[mode] = st
                e[f"order_{o}"] = entry
            row[v] = e
        rec["rows"][str(S)] = row
    if a.parent_lib:
        rec["rows_within_parent_min_max"] = f"{within} of {total}"
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
