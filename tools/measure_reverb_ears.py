#!/usr/bin/env python3
"""Two-ear late reverb (fs_reverb_set_ears): host wall time of one fs_reverb_process_batch that serves S partitioned sources
with ears against the same call for S partitioned sources without, and the rows without ears against a library built from the
PARENT commit.

  * 1024 stereo frames, 48 000 samples, 8 bands; S in {1, 32, 128}; three variants: a take in every callback (a new installed
    IR before each, no crossfade), no take (a constant IR), a running crossfade (a fade of 4 s, started by one untimed
    callback and re-started before it runs out, so that every timed callback forms both products and none takes);
  * ears against mono: the two series alternate, one process per repeat; reported is ears / mono of the medians over all
    repeats.  No ratio is fixed in advance: the ear MAC reads twice the H bytes and the X ring twice;
  * mono rows, this build against the parent's (--parent-lib): --repeats processes each, alternating; a row passes when the
    median of this build's per-process medians lies within the min - max of the parent's (DESIGN.md section 8's rule), and
    the output digests are equal.

usage: python tools/measure_reverb_ears.py --parent-lib PATH [--callbacks 200] [--repeats 5] [--out profiles/reverb_ears.json]"""
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

FRAME, BANDS, SIZES = 1024, 8, (1, 32, 128)
VARIANTS = ("take_every_callback", "no_take", "running_crossfade")
LONG_FADE = 4 * 48000          # the longest fs_reverb_set_crossfade takes: 187 callbacks of 1024
RESTART = 150                  # timed callbacks between two installs of the running-crossfade variant
PARTITIONED = 1


class Lib:
    """the entry points the measurement needs, bound to ONE library file, on an 8-band context"""

    def __init__(self, path, capi):
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
        lib = C.CDLL(path)
        vp, i32 = C.c_void_p, C.c_int32
        lib.fs_config_default.argtypes = [C.POINTER(capi.Config)]
        lib.fs_config_default.restype = None
        sigs = [("fs_context_create", [C.POINTER(capi.Config), C.POINTER(vp)]), ("fs_context_destroy", [vp]),
                ("fs_source_create", [vp, C.POINTER(i32)]), ("fs_num_samples", [vp]), ("fs_reverb_init", [vp, i32, i32]),
                ("fs_reverb_set_crossfade", [vp, i32, i32]), ("fs_reverb_set_engine", [vp, i32, i32]),
                ("fs_set_impulse_response", [vp, i32, vp, i32]),
                ("fs_reverb_process_batch", [vp, vp, i32, vp, vp, vp, C.c_uint32, vp])]
        self.has_ears = hasattr(lib, "fs_reverb_set_ears")
        if self.has_ears:
            sigs += [("fs_reverb_ears_set", [vp, vp]), ("fs_reverb_set_ears", [vp, i32, i32])]
        for name, args in sigs:
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = C.c_int
        lib.fs_last_error.argtypes = [vp]
        lib.fs_last_error.restype = C.c_char_p
        self.lib = lib
        cfg = capi.Config()
        lib.fs_config_default(C.byref(cfg))
        cfg.num_bands = BANDS
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


def series_times(lib, capi, ears, callbacks, warmup):
    """{S: {variant: {"times": [seconds per callback], "sha256": of the timed outputs}}}; same seeded inputs and IRs whatever the series"""
    rng = np.random.default_rng(0)
    irs = [mb.noise_ir(rng, lib.n) for _ in range(4)]
    if ears:
        d = capi.default_reverb_ears()
        lib.ok(lib.lib.fs_reverb_ears_set(lib.h, C.addressof(d)))
    pools = {}
    for v in VARIANTS:
        pool = [lib.source() for _ in range(max(SIZES))]
        for s in pool:
            lib.ok(lib.lib.fs_reverb_set_engine(lib.h, s, PARTITIONED))
            if ears:
                lib.ok(lib.lib.fs_reverb_set_ears(lib.h, s, 1))
            if v == "running_crossfade":
                lib.ok(lib.lib.fs_reverb_set_crossfade(lib.h, s, LONG_FADE))
            lib.ok(lib.lib.fs_reverb_init(lib.h, s, FRAME))
            lib.ok(lib.lib.fs_set_impulse_response(lib.h, s, irs[0].ctypes.data, lib.n))
        pools[v] = pool
    res = {}
    for S in SIZES:
        blk = np.clip(rng.normal(0, 0.3, (S, 2 * FRAME)), -1, 1).astype(np.float32)
        out = np.empty_like(blk)
        for v in VARIANTS:
            srcs = np.array(pools[v][:S], np.int32)

            def call():
                t = time.perf_counter()
                rc = lib.lib.fs_reverb_process_batch(lib.h, srcs.ctypes.data, S, blk.ctypes.data, out.ctypes.data, None, 0, None)
                dt = time.perf_counter() - t
                lib.ok(rc)
                return dt

            def install(k):
                for s in srcs:
                    lib.ok(lib.lib.fs_set_impulse_response(lib.h, int(s), irs[k % 4].ctypes.data, lib.n))

            times, sha = [], hashlib.sha256()
            for i in range(warmup + callbacks):
                if v == "take_every_callback":
                    install(i)
                elif v == "running_crossfade" and (i == 0 or (i >= warmup and (i - warmup) % RESTART == 0)):
                    call()              # (the first callback after fs_reverb_init takes unfaded: there is something to fade from)
                    install(i + 1)
                    call()              # the take that starts the fade: untimed
                dt = call()
                if i >= warmup:
                    times.append(dt)
                    sha.update(out.tobytes())
            res.setdefault(str(S), {})[v] = {"times": times, "sha256": sha.hexdigest()}
    return res


def run_worker(path, ears, callbacks, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", path, "--ears", str(int(ears)), "--callbacks", str(callbacks),
           "--warmup", str(warmup)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if p.returncode or not line:
        sys.exit(f"{cmd} failed with status {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libfrequensee.so built from the parent commit")
    ap.add_argument("--callbacks", type=int, default=200, help="timed callbacks per process, size and variant")
    ap.add_argument("--repeats", type=int, default=5, help="processes per series")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--ears", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    capi = mb.graft.load_package()._capi
    this_lib = capi.LIB_PATH
    if a.worker:
        lib = Lib(a.lib, capi)
        res = series_times(lib, capi, bool(a.ears), a.callbacks, a.warmup)
        lib.close()
        print("RESULT " + json.dumps(res))
        return 0
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libfrequensee.so built from the parent commit is the baseline of this measurement")
    series = (("parent_mono", a.parent_lib, False), ("this_mono", this_lib, False), ("this_ears", this_lib, True))
    raw = {name: {} for name, _, _ in series}      # [name][S][variant] -> list of per-process time lists
    bits = {name: {} for name, _, _ in series}
    for r in range(a.repeats):
        for name, path, ears in series:
            for S, vs in run_worker(path, ears, a.callbacks, a.warmup).items():
                for v, got in vs.items():
                    raw[name].setdefault(S, {}).setdefault(v, []).append(got["times"])
                    bits[name].setdefault(S, {}).setdefault(v, set()).add(got["sha256"])
            print(f"repeat {r} {name} done", file=sys.stderr, flush=True)
    rec = {"callback": f"one fs_reverb_process_batch, {FRAME} stereo frames, 48000 samples, {BANDS} bands, partitioned engine",
           "repeats": a.repeats, "callbacks_per_process": a.callbacks, "rows": {}}
    within = 0
    for S in SIZES:
        row = {}
        for v in VARIANTS:
            e = {name: mb.stats(np.concatenate(raw[name][str(S)][v])) for name, _, _ in series}
            pm = [float(np.median(t)) * 1e3 for t in raw["parent_mono"][str(S)][v]]
            hm = [float(np.median(t)) * 1e3 for t in raw["this_mono"][str(S)][v]]
            e["ears_over_mono"] = e["this_ears"]["median_ms"] / e["this_mono"]["median_ms"]
            e["parent_mono_process_medians_ms"], e["this_mono_process_medians_ms"] = pm, hm
            e["this_mono_median_of_medians_ms"] = float(np.median(hm))
            e["mono_within_parent_min_max"] = bool(min(pm) <= float(np.median(hm)) <= max(pm))
            e["mono_over_parent"] = float(np.median(hm)) / float(np.median(pm))
            e["mono_bits_equal_parent"] = bits["this_mono"][str(S)][v] == bits["parent_mono"][str(S)][v] and len(bits["this_mono"][str(S)][v]) == 1
            within += e["mono_within_parent_min_max"]
            row[v] = e
        rec["rows"][str(S)] = row
    rec["mono_rows_within_parent_min_max"] = f"{within} of {len(SIZES) * len(VARIANTS)}"
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
