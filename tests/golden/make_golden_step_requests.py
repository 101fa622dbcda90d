"""Writes tests/golden/step_requests_<scene>.npz: closest hits and any hits of one wave of signed-zero and mixed-sign
rays, and one deterministic frame's energy (tests/test_step_requests.py: record), for the two test scenes and the two
degenerate ones.  Run ONCE, on the GPU, with the build whose results are the reference — the commit before the step's
requests and direction signs changed — and not again afterwards:
    python tests/golden/make_golden_step_requests.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root

import __graft_entry__ as graft  # noqa: E402
import test_step_requests as T  # noqa: E402


def main(out_dir=T.GOLDEN_DIR):
    os.environ.pop("FS_STACK_ROWS_CAP", None)
    pkg = graft.load_package()
    scenes = [(name, pkg.scenes.by_name(name, bands)) for name, bands in T.SCENES.items()]
    scenes += [(name, T.degenerate_scene(pkg, name)) for name in T.DEGENERATE]
    for name, sc in scenes:
        got = T.record(pkg, sc)
        path = os.path.join(out_dir, os.path.basename(T.golden_path(name)))
        np.savez_compressed(path, **got)
        print(f"{path}: {os.path.getsize(path)} bytes, hit {got['hit'].mean():.3f}, any_hit {got['any_hit'].mean():.3f}, "
              f"energy bins {int((got['energy'] != 0).sum())}, energy sum {float(got['energy'].sum()):.6g}")
        if name in T.SCENES:
            T.check_fractions(name, got)   # both hits and misses, or the recording is not kept


if __name__ == "__main__":
    main(*sys.argv[1:2])
