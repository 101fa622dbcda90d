"""Writes tests/golden/python_record_layouts.json and tests/golden/path_voices.npz (tests/test_python_goldens.py: layouts,
synthetic, voices).  Run ONCE, at a commit whose Python facade is the reference — the last one whose dtypes were written by
hand and whose Voices() walked the path kinds by a running index — and not again with the code the files check:
    python tests/golden/make_golden_python_facade.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root

import __graft_entry__ as graft  # noqa: E402
import test_python_goldens as T  # noqa: E402


def main(out_dir=T.GOLDEN):
    pkg = graft.load_package()
    with open(os.path.join(out_dir, "python_record_layouts.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(T.layouts(pkg.Context).items())) + "\n}\n")   # a line per dtype
    data, pathing, direct = T.synthetic(pkg)
    arrays = {"in_pathing": pathing.view(np.uint8), "in_direct": direct.view(np.uint8)}
    for kind, (rows, paths) in data.items():
        arrays[f"in_{kind}_rows"] = rows.view(np.uint8)
        arrays[f"in_{kind}_paths"] = paths.view(np.uint8).reshape(2, -1)
    for name, v in T.voices(pkg, data, pathing, direct).items():
        arrays[f"out_{name}"] = v.view(np.uint8)
    np.savez_compressed(os.path.join(out_dir, "path_voices.npz"), **arrays)
    print({k: v.shape for k, v in arrays.items() if k.startswith("out_")})


if __name__ == "__main__":
    main(*sys.argv[1:2])
