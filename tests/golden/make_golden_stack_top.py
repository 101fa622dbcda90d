"""Writes tests/golden/stack_top_<scene>_rays_and_energy.npz: closest hits, any hits and one deterministic frame's energy
of seeded queries (tests/test_stack_top_cache.py: record).  Run ONCE, on the GPU, with the build whose results are the
reference — the commit before the stack-top experiment — and not again afterwards:
    python tests/golden/make_golden_stack_top.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root

import __graft_entry__ as graft  # noqa: E402
import test_stack_top_cache as T  # noqa: E402


def main(out_dir=T.GOLDEN_DIR):
    os.environ.pop("FS_STACK_ROWS_CAP", None)
    pkg = graft.load_package()
    for name, bands in T.SCENES.items():
        got = T.record(pkg, pkg.scenes.by_name(name, bands))
        path = os.path.join(out_dir, os.path.basename(T.golden_path(name)))
        np.savez_compressed(path, **got)
        print(f"{path}: {os.path.getsize(path)} bytes, hit {got['hit'].mean():.3f}, any_hit {got['any_hit'].mean():.3f}, "
              f"energy bins {int((got['energy'] != 0).sum())}")


if __name__ == "__main__":
    main(*sys.argv[1:2])
