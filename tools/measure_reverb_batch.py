#!/usr/bin/env python3
"""Row f2 for many sources: host wall time of one audio callback that serves S sources, as the per-source loop of
fs_reverb_process and as one fs_reverb_process_batch — on this build and on a library built from the PARENT commit, whose
numbers are the baselines and whose output bits this build must reproduce.

  * S in {1, 2, 8, 32, 128}, 1024 stereo frames, 48 000-tap installed IRs, three cases each: no crossfade; crossfade (2560
    samples) with constant IRs; crossfade with a new IR for every source before every callback (the installs are not timed);
  * four series: the loop and the batch on a library built from the PARENT commit (--parent-lib, a second build tree:
    tools/build_variant.sh in a checkout of the parent), the loop and the batch on this build.  Every series runs in a process
    of its own, the series alternate in rounds, and a callback's time is the host clock around the call (which ends in the
    stream synchronise the audio thread waits for);
  * per series the median and the 10th / 90th percentile over all timed callbacks (>= 500 after a warm-up).  What must hold per
    entry: this build's loop <= 1.07 x the parent's loop, this build's batch <= 1.07 x the parent's batch (medians; 7 % is the
    spread already seen between sessions for the single call, 0.100 vs 0.107 ms);
  * every series draws the same inputs and installs the same IRs (one seed), and returns a SHA-256 over all outputs of its
    timed callbacks per size and case: this build's loop and batch must both equal the parent's loop (bits_equal_parent).

Without a GPU the tool fails (the context cannot be created); nothing falls back.
--profile-run: a short run of batch callbacks for S = 1 and S = 128 (plain, then fading with a new IR every callback), for
`rocprofv3 --kernel-trace --stats -- python tools/measure_reverb_batch.py --profile-run` (launch counts and kernel times).
usage: python tools/measure_reverb_batch.py --parent-lib PATH [--callbacks 500] [--rounds 2] [--out profiles/reverb_unified.json]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

FRAME = 1024
FADE = 2560
SIZES = (1, 2, 8, 32, 128)
CASES = ("no_crossfade", "crossfade_constant_ir", "crossfade_new_ir_every_callback")
SERIES = ("parent_loop", "parent_batch", "this_loop", "this_batch")


def noise_ir(rng, n):
    return (rng.normal(0, 1, n) * np.exp(-np.arange(n) / 5000.0) * 0.02).astype(np.float32)


class Lib:
    """the few entry points the measurement needs, bound to ONE library file (the package binds its own build only)"""

    def __init__(self, path, capi):
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
        lib = C.CDLL(path)
        vp, i32 = C.c_void_p, C.c_int32
        lib.fs_config_default.argtypes = [C.POINTER(capi.Config)]
        lib.fs_config_default.restype = None
        for name, args in (("fs_context_create", [C.POINTER(capi.Config), C.POINTER(vp)]), ("fs_context_destroy", [vp]),
                           ("fs_source_create", [vp, C.POINTER(i32)]), ("fs_num_samples", [vp]), ("fs_reverb_init", [vp, i32, i32]),
                           ("fs_reverb_set_crossfade", [vp, i32, i32]), ("fs_set_impulse_response", [vp, i32, vp, i32]),
                           ("fs_reverb_process", [vp, i32, vp, vp, i32, C.c_uint32])):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = C.c_int
        lib.fs_last_error.argtypes = [vp]
        lib.fs_last_error.restype = C.c_char_p
        self.has_batch = hasattr(lib, "fs_reverb_process_batch")
        if self.has_batch:
            lib.fs_reverb_process_batch.argtypes = [vp, vp, i32, vp, vp, vp, C.c_uint32, vp]
            lib.fs_reverb_process_batch.restype = C.c_int
        self.lib = lib
        cfg = capi.Config()
        lib.fs_config_default(C.byref(cfg))
        cfg.num_bands = 1
        self.h = vp()
        rc = lib.fs_context_create(C.byref(cfg), C.byref(self.h))
        if rc:
            msg = lib.fs_last_error(self.h).decode() if self.h else "fs_context_create failed"
            raise RuntimeError(f"{path}: status {rc}: {msg} (this measurement needs the GPU)")
        self.n = lib.fs_num_samples(self.h)

    def ok(self, rc):
        if rc:
            raise RuntimeError(f"status {rc}: {self.lib.fs_last_error(self.h).decode()}")

    def source(self):
        s = C.c_int32(-1)
        self.ok(self.lib.fs_source_create(self.h, C.byref(s)))
        return s.value

    def close(self):
        self.lib.fs_context_destroy(self.h)


def series_times(lib, batch, callbacks, warmup, sizes=SIZES, cases=CASES):
    """{S: {case: {"times": [seconds per callback], "sha256": of the timed callbacks' outputs}}}: sources are created once per
    case (3 x 128), the first S of them serve size S; inputs and IRs come from one seed, whatever the series"""
    rng = np.random.default_rng(0)
    irs = [noise_ir(rng, lib.n) for _ in range(4)]
    res = {}
    pools = {}
    for case in cases:
        pool = [lib.source() for _ in range(max(sizes))]
        for s in pool:
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
                if batch:
                    t = time.perf_counter()
                    rc = lib.lib.fs_reverb_process_batch(lib.h, srcs.ctypes.data, S, blk.ctypes.data, out.ctypes.data, None, 0, None)
                    dt = time.perf_counter() - t
                    lib.ok(rc)
                else:
                    rcs = 0
                    t = time.perf_counter()
                    for k in range(S):
                        rcs |= lib.lib.fs_reverb_process(lib.h, int(srcs[k]), blk[k].ctypes.data, out[k].ctypes.data, 1, 0)
                    dt = time.perf_counter() - t
                    lib.ok(rcs)
                if i >= warmup:
                    times.append(dt)
                    sha.update(out.tobytes())
            res.setdefault(str(S), {})[case] = {"times": times, "sha256": sha.hexdigest()}
    return res


def worker(a, capi):
    lib = Lib(a.lib, capi)
    if a.batch and not lib.has_batch:
        raise RuntimeError(f"{a.lib} has no fs_reverb_process_batch")
    res = series_times(lib, a.batch, a.callbacks, a.warmup)
    lib.close()
    print("RESULT " + json.dumps(res))


def profile_run(capi, this_lib, callbacks=20):
    lib = Lib(this_lib, capi)
    series_times(lib, True, callbacks, 2, sizes=(1, 128), cases=("no_crossfade", "crossfade_new_ir_every_callback"))
    lib.close()
    print(json.dumps({"profile_run": {"callbacks_per_size_and_case": callbacks + 2, "sizes": [1, 128]}}))


def stats(ts):
    ms = 1e3 * np.asarray(ts)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "mean_ms": float(ms.mean()), "callbacks": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libfrequensee.so built from the parent commit")
    ap.add_argument("--callbacks", type=int, default=500, help="timed callbacks per series, size and case, over all rounds")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--batch", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    capi = graft.load_package()._capi
    this_lib = capi.LIB_PATH
    if a.worker:
        worker(a, capi)
        return 0
    if a.profile_run:
        profile_run(capi, this_lib)
        return 0
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libfrequensee.so built from the parent commit is the baseline of this measurement")
    per_round = (a.callbacks + a.rounds - 1) // a.rounds
    raw = {name: {} for name in SERIES}
    bits = {name: {} for name in SERIES}   # [S][case]: the rounds' digests, in order
    for r in range(a.rounds):
        for name, path, batch in (("parent_loop", a.parent_lib, False), ("parent_batch", a.parent_lib, True),
                                  ("this_loop", this_lib, False), ("this_batch", this_lib, True)):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", path, "--callbacks", str(per_round), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd + (["--batch"] if batch else []), capture_output=True, text=True, timeout=900)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode or not line:
                sys.exit(f"{name} (round {r}) failed with status {p.returncode}:\n{p.stderr[-2000:]}")
            for S, cases in json.loads(line[0][7:]).items():
                for case, got in cases.items():
                    raw[name].setdefault(S, {}).setdefault(case, []).extend(got["times"])
                    bits[name].setdefault(S, {}).setdefault(case, []).append(got["sha256"])
            print(f"round {r} {name} done", file=sys.stderr, flush=True)
    rec = {"callback": f"{FRAME} stereo frames, 48000-tap installed IRs, crossfade {FADE} samples", "rounds": a.rounds, "sizes": {}}
    holds = True
    for S in SIZES:
        row = {}
        for case in CASES:
            e = {name: stats(raw[name][str(S)][case]) for name in SERIES}
            e["this_loop_over_parent_loop"] = e["this_loop"]["median_ms"] / e["parent_loop"]["median_ms"]
            e["this_batch_over_parent_batch"] = e["this_batch"]["median_ms"] / e["parent_batch"]["median_ms"]
            want = bits["parent_loop"][str(S)][case]
            e["sha256"] = want
            e["bits_equal_parent"] = {name: bits[name][str(S)][case] == want for name in ("this_loop", "this_batch")}
            # what must hold: each path within 7 % of the PARENT's same path, and the parent loop's bits from both
            e["holds"] = bool(e["this_loop_over_parent_loop"] <= 1.07 and e["this_batch_over_parent_batch"] <= 1.07
                              and all(e["bits_equal_parent"].values()))
            holds = holds and e["holds"]
            row[case] = e
        rec["sizes"][str(S)] = row
    rec["all_hold"] = holds
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if holds else 1


if __name__ == "__main__":
    sys.exit(main())
