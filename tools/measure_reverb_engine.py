#!/usr/bin/env python3
"""Row f2, the two reverb engines: host wall time of one fs_reverb_process_batch that serves S sources with the direct engine
and with the partitioned one (fs_reverb_set_engine), and the direct engine against a library built from the PARENT commit.

  * S in {1, 2, 8, 32, 128}, 1024 stereo frames, 48 000-tap installed IRs, the three cases of tools/measure_reverb_batch.py
    (same seeded inputs and IRs, same clock: the host's, around the call);
  * three series: the batch on the parent's library (--parent-lib), the batch on this build with the direct engine, the batch
    on this build with the partitioned engine.  Every series runs in a process of its own and the series alternate in rounds;
  * per series the median and the 10th / 90th percentile over all timed callbacks.  What must hold: from S = 8 up the
    partitioned median is not above the direct median (no margin: the arithmetic is two orders of magnitude smaller), and the
    direct engine's median on this build is <= 1.07 x the parent's in every entry, with the parent's output bits;
  * --long SECONDS: S = 8 on a context of that simulated duration at 48 kHz (partitioned only: the direct engine refuses IRs
    beyond its history ring), reported, or the status fs_context_create refuses it with.

--profile-run: a short run of partitioned batch callbacks for S = 1 and S = 128 (plain, then fading with a new IR every
callback), for `rocprofv3 --kernel-trace --stats -- python tools/measure_reverb_engine.py --profile-run`.
usage: python tools/measure_reverb_engine.py --parent-lib PATH [--callbacks 300] [--rounds 2] [--long 4.0] [--out profiles/reverb_partitioned.json]"""
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

FRAME, FADE, SIZES, CASES = mb.FRAME, mb.FADE, mb.SIZES, mb.CASES
SERIES = ("parent_direct", "this_direct", "this_partitioned")
PARTITIONED = 1


class Lib(mb.Lib):
    def __init__(self, path, capi):
        super().__init__(path, capi)
        if hasattr(self.lib, "fs_reverb_set_engine"):
            self.lib.fs_reverb_set_engine.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
            self.lib.fs_reverb_set_engine.restype = C.c_int


def long_context(path, capi, seconds):
    """(a Lib whose context simulates `seconds` at the default sample rate, 0), or (None, the status it was refused with)"""
    lib = Lib(path, capi)
    lib.close()                        # the default context: only its bindings are kept
    cfg = capi.Config()
    lib.lib.fs_config_default(C.byref(cfg))
    cfg.num_bands = 1
    cfg.simulated_duration = seconds
    lib.h = C.c_void_p()
    rc = lib.lib.fs_context_create(C.byref(cfg), C.byref(lib.h))
    if rc:
        return None, rc
    lib.n = lib.lib.fs_num_samples(lib.h)
    return lib, 0


def series_times(lib, engine, callbacks, warmup, sizes=SIZES, cases=CASES):
    """measure_reverb_batch.series_times for the batch, the sources initialised with `engine`"""
    rng = np.random.default_rng(0)
    irs = [mb.noise_ir(rng, lib.n) for _ in range(4)]
    res, pools = {}, {}
    for case in cases:
        pool = [lib.source() for _ in range(max(sizes))]
        for s in pool:
            if engine:
                lib.ok(lib.lib.fs_reverb_set_engine(lib.h, s, engine))
            lib.ok(lib.lib.fs_reverb_init(lib.h, s, FRAME))
            if case != "no_crossfade":
                lib.ok(lib.lib.fs_reverb_set_crossfade(lib.h, s, FADE))
            lib.ok(lib.lib.fs_set_impulse_response(lib.h, s, irs[0].ctypes.data, lib.n))
        pools[case] = pool
    for S in sizes:
        blk = np.clip(rng.normal(0, 0.3, (S, 2 * FRAME)), -1, 1).astype(np.float32)
        out = np.empty_like(blk)
        for case in cases:
            srcs = np.array(pools[case][:S], np.int32)
            times, sha = [], hashlib.sha256()
            for i in range(warmup + callbacks):
                if case == "crossfade_new_ir_every_callback":
                    for s in srcs:
                        lib.ok(lib.lib.fs_set_impulse_response(lib.h, int(s), irs[i % 4].ctypes.data, lib.n))
                t = time.perf_counter()
                rc = lib.lib.fs_reverb_process_batch(lib.h, srcs.ctypes.data, S, blk.ctypes.data, out.ctypes.data, None, 0, None)
                dt = time.perf_counter() - t
                lib.ok(rc)
                if i >= warmup:
                    times.append(dt)
                    sha.update(out.tobytes())
            res.setdefault(str(S), {})[case] = {"times": times, "sha256": sha.hexdigest()}
    return res


def worker(a, capi):
    if a.long:
        lib, rc = long_context(a.lib, capi, a.long)
        if lib is None:
            print("RESULT " + json.dumps({"refused": rc}))
            return
        res = series_times(lib, PARTITIONED, a.callbacks, a.warmup, sizes=(8,))
        res["num_samples"] = lib.n
    else:
        lib = Lib(a.lib, capi)
        res = series_times(lib, a.engine, a.callbacks, a.warmup)
    lib.close()
    print("RESULT " + json.dumps(res))


def run_worker(path, engine, callbacks, warmup, long=0.0):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", path, "--engine", str(engine), "--callbacks", str(callbacks),
           "--warmup", str(warmup), "--long", str(long)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if p.returncode or not line:
        sys.exit(f"{cmd} failed with status {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libfrequensee.so built from the parent commit")
    ap.add_argument("--callbacks", type=int, default=300, help="timed callbacks per series, size and case, over all rounds")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--long", type=float, default=0.0, help="also S = 8 on a context of this many seconds (partitioned)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--engine", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    capi = mb.graft.load_package()._capi
    this_lib = capi.LIB_PATH
    if a.worker:
        worker(a, capi)
        return 0
    if a.profile_run:
        lib = Lib(this_lib, capi)
        series_times(lib, PARTITIONED, 20, 2, sizes=(1, 128), cases=("no_crossfade", "crossfade_new_ir_every_callback"))
        lib.close()
        print(json.dumps({"profile_run": {"callbacks_per_size_and_case": 22, "sizes": [1, 128], "engine": "partitioned"}}))
        return 0
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libfrequensee.so built from the parent commit is the baseline of this measurement")
    per_round = (a.callbacks + a.rounds - 1) // a.rounds
    raw = {name: {} for name in SERIES}
    bits = {name: {} for name in SERIES}
    for r in range(a.rounds):
        for name, path, engine in (("parent_direct", a.parent_lib, 0), ("this_direct", this_lib, 0), ("this_partitioned", this_lib, PARTITIONED)):
            for S, cases in run_worker(path, engine, per_round, a.warmup).items():
                for case, got in cases.items():
                    raw[name].setdefault(S, {}).setdefault(case, []).extend(got["times"])
                    bits[name].setdefault(S, {}).setdefault(case, []).append(got["sha256"])
            print(f"round {r} {name} done", file=sys.stderr, flush=True)
    rec = {"callback": f"one fs_reverb_process_batch, {FRAME} stereo frames, 48000-tap installed IRs, crossfade {FADE} samples",
           "rounds": a.rounds, "sizes": {}}
    holds = True
    for S in SIZES:
        row = {}
        for case in CASES:
            e = {name: mb.stats(raw[name][str(S)][case]) for name in SERIES}
            e["partitioned_over_direct"] = e["this_partitioned"]["median_ms"] / e["this_direct"]["median_ms"]
            e["direct_over_parent"] = e["this_direct"]["median_ms"] / e["parent_direct"]["median_ms"]
            e["direct_bits_equal_parent"] = bits["this_direct"][str(S)][case] == bits["parent_direct"][str(S)][case]
            e["partitioned_gated"] = S >= 8
            e["holds"] = bool((S < 8 or e["partitioned_over_direct"] <= 1.0) and e["direct_over_parent"] <= 1.07 and e["direct_bits_equal_parent"])
            holds = holds and e["holds"]
            row[case] = e
        rec["sizes"][str(S)] = row
    if a.long:
        got = run_worker(this_lib, PARTITIONED, a.callbacks, a.warmup, a.long)
        if "refused" in got:
            rec["long_context"] = {"seconds": a.long, "fs_context_create_status": got["refused"]}
        else:
            rec["long_context"] = {"seconds": a.long, "num_samples": got["num_samples"], "S": 8,
                                   "partitioned": {case: mb.stats(v["times"]) for case, v in got["8"].items()}}
    rec["all_hold"] = holds
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if holds else 1


if __name__ == "__main__":
    sys.exit(main())
