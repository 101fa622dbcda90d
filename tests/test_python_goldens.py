"""The Python facade against two files recorded once, at the last commit that wrote every record layout by hand
(tests/golden/make_golden_python_facade.py): Context's dtypes, which are derived from the ctypes structures, and what the
Voices() of the two voice plugins make of path records of all kinds at once.  No device is needed.

python_record_layouts.json: per Context.*_DTYPE the fields as [name, offset, base type string, shape] and the itemsize.
path_voices.npz: a seeded synthetic input (rows and paths of the five listed kinds for two sources, three pathing rows, two
direct rows), as bytes, and the bytes FrequenSeeAudioReflectionPlugin.Voices and FrequenSeeAudioBinauralPlugin.Voices return.
"""
import json
import os

import numpy as np
import pytest

from test_reflection_render import _Ctx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("reflection", "diffraction", "second", "diffraction2", "mixed")
# returned paths per source and kind; source 0 fills a bank of 32 voices: 10 + 6 + (7 - 1) + (5 - 1) + (6 - 1) + 1 pathing voice
RETURNED = dict(reflection=(10, 3), diffraction=(6, 2), second=(7, 2), diffraction2=(5, 1), mixed=(6, 0))
CAPACITY = dict(reflection=12, diffraction=8, second=8, diffraction2=6, mixed=8)
COLLIDE = dict(second=(1, 4), diffraction2=(0, 3), mixed=(2, 5))   # (keep, drop): source 0's path [drop] has path [keep]'s identity


def layouts(ctx_cls):
    out = {}
    for name in sorted(n for n in vars(ctx_cls) if n.endswith("_DTYPE")):
        dt = getattr(ctx_cls, name)
        out[name] = dict(itemsize=dt.itemsize,
                         fields=[[k, dt.fields[k][1], dt.fields[k][0].base.str, list(dt.fields[k][0].shape)] for k in dt.names])
    return out


def path_dtypes(ctx_cls):
    return dict(reflection=(ctx_cls.REFLECTION_ROW_DTYPE, ctx_cls.REFLECTION_DTYPE), diffraction=(ctx_cls.DIFFRACTION_ROW_DTYPE, ctx_cls.DIFFRACTION_DTYPE),
                second=(ctx_cls.REFLECTION2_ROW_DTYPE, ctx_cls.REFLECTION2_DTYPE), diffraction2=(ctx_cls.DIFFRACTION2_ROW_DTYPE, ctx_cls.DIFFRACTION2_DTYPE),
                mixed=(ctx_cls.MIXED_ROW_DTYPE, ctx_cls.MIXED_DTYPE))


def synthetic(pkg):
    """(dict kind -> (rows [2], paths [2][capacity]), pathing rows [3]: found, found and DIRECT, not found, direct rows [2])"""
    cap, ctx_cls = pkg._capi, pkg.Context
    rng = np.random.default_rng(0x601DE2)
    dtypes = path_dtypes(ctx_cls)

    def fill(a):
        """every field of the records a: floats in a plausible range, unit directions, distinct small indices"""
        for k in a.dtype.names:
            shape = a[k].shape
            if k == "direction" or k == "departure":
                d = rng.normal(size=shape)
                a[k] = d / np.linalg.norm(d, axis=-1, keepdims=True)
            elif k in ("length", "distance"):
                a[k] = rng.uniform(100.0, 900.0, shape)
            elif k == "delay":
                a[k] = rng.uniform(0.0, 0.03, shape)   # some below the band filter's latency of 127 samples
            elif k == "triangle":
                a[k] = rng.permutation(100000)[:int(np.prod(shape))].reshape(shape)
            elif k in ("edge", "hops"):
                a[k] = rng.integers(0, 3, shape)
            elif k == "end":
                a[k] = rng.integers(0, 2, shape)
            elif a[k].dtype.kind == "f":
                a[k] = rng.uniform(0.0, 1.0, shape)
            else:
                a[k] = rng.integers(0, 16, shape)
        return a

    data = {}
    for kind in KINDS:
        rows = np.zeros(2, dtype=dtypes[kind][0])
        paths = fill(np.zeros((2, CAPACITY[kind]), dtype=dtypes[kind][1]))
        rows["returned"] = RETURNED[kind]
        rows["found"] = rows["returned"]
        if kind in COLLIDE:
            keep, drop = COLLIDE[kind]
            for k in ("triangle", "edge", "end"):
                if k in paths.dtype.names:
                    paths[0, drop][k] = paths[0, keep][k]
        data[kind] = (rows, paths)
    pathing = fill(np.zeros(3, dtype=ctx_cls.PATHING_DTYPE))
    pathing["flags"] = [cap.PATHING_FOUND | cap.PATHING_STALE, cap.PATHING_FOUND | cap.PATHING_DIRECT, 0]
    direct = fill(np.zeros(2, dtype=ctx_cls.DIRECT_DTYPE))
    return data, pathing, direct


RIGHT, FORWARD = [0.6, 0.8, 0.0], [0.8, -0.6, 0.0]
REFERENCE_LENGTH = 300.0
TO_SOURCE = [[410.0, -330.0, 60.0], [-20.0, 15.0, 5.0]]
CALLS = ((0, 0), (1, 1), (1, 2))   # (source, pathing row)


def plugin(cls):
    plug = cls.__new__(cls)
    plug.ctx, plug.Taps = _Ctx, 255
    return plug


def voices(pkg, data, pathing, direct):
    """dict name -> the array a Voices call returns: every (source, pathing row) of CALLS with all kinds, and source 0 with each
    optional kind alone"""
    refl, bina = plugin(pkg.FrequenSeeAudioReflectionPlugin), plugin(pkg.FrequenSeeAudioBinauralPlugin)

    def pick(kind, s):
        return data[kind][0][s], data[kind][1][s]

    out = {}
    for s, pr in CALLS:
        row, paths = pick("reflection", s)
        kw = dict({k: pick(k, s) for k in KINDS[1:]}, pathing=pathing[pr])
        out[f"reflection_{s}_{pr}"] = refl.Voices(row, paths, right=RIGHT, reference_length=REFERENCE_LENGTH, **kw)
        out[f"binaural_{s}_{pr}"] = bina.Voices(row, paths, FORWARD, RIGHT, reference_length=REFERENCE_LENGTH, **kw)
        out[f"binaural_direct_{s}_{pr}"] = bina.Voices(row, paths, FORWARD, RIGHT, direct=(direct[s], TO_SOURCE[s]), **kw)
    row, paths = pick("reflection", 0)
    out["reflection_plain"] = refl.Voices(row, paths)
    for k in KINDS[1:]:
        out[f"reflection_only_{k}"] = refl.Voices(row, paths, right=RIGHT, **{k: pick(k, 0)})
    out["reflection_only_pathing"] = refl.Voices(row, paths, pathing=pathing[0])
    return out


def test_record_layouts(pkg):
    recorded = json.load(open(os.path.join(GOLDEN, "python_record_layouts.json")))
    assert sorted(recorded) == sorted(n for n in vars(pkg.Context) if n.endswith("_DTYPE"))
    for name, want in recorded.items():
        dt = getattr(pkg.Context, name)
        assert dt.itemsize == want["itemsize"], name
        assert list(dt.names) == [f[0] for f in want["fields"]], name
        for k, offset, base, shape in want["fields"]:
            sub, off = dt.fields[k][:2]
            assert (off, sub.base.str, list(sub.shape)) == (offset, base, shape), (name, k)
        assert dt == np.dtype([(k, base, tuple(shape)) for k, _, base, shape in want["fields"]]), name
    assert pkg.Context.AMBISONIC_VOICE_DTYPE is pkg.Context.BINAURAL_VOICE_DTYPE


def recorded_input(pkg):
    z = np.load(os.path.join(GOLDEN, "path_voices.npz"))
    ctx_cls = pkg.Context
    dtypes = path_dtypes(ctx_cls)
    data = {k: (z[f"in_{k}_rows"].view(r), z[f"in_{k}_paths"].view(p)) for k, (r, p) in dtypes.items()}
    return z, data, z["in_pathing"].view(ctx_cls.PATHING_DTYPE), z["in_direct"].view(ctx_cls.DIRECT_DTYPE)


def test_path_voices(pkg):
    cap = pkg._capi
    z, data, pathing, direct = recorded_input(pkg)
    # the input is what its description says: colliding keys in the three kinds that drop them, the three pathing states
    plug = plugin(pkg.FrequenSeeAudioReflectionPlugin)
    for kind, (keep, drop) in COLLIDE.items():
        p = data[kind][1][0]
        key = dict(second=lambda q: plug.SecondOrderKey(q["triangle"][0], q["triangle"][1]), diffraction2=lambda q: plug.Diffraction2Key(q["triangle"], q["edge"]),
                   mixed=lambda q: plug.MixedKey(q["triangle"], q["edge"], q["end"]))[kind]
        assert key(p[keep]) == key(p[drop]) and drop < data[kind][0][0]["returned"] and p[keep]["delay"] != p[drop]["delay"], kind
    found = pathing["flags"] & (cap.PATHING_FOUND | cap.PATHING_DIRECT)
    assert list(found) == [cap.PATHING_FOUND, cap.PATHING_FOUND | cap.PATHING_DIRECT, 0]
    got = voices(pkg, data, pathing, direct)
    assert sorted("out_" + k for k in got) == sorted(k for k in z.files if k.startswith("out_"))
    for name, v in got.items():
        assert v.tobytes() == z["out_" + name].tobytes(), name
    assert len(got["reflection_0_0"]) == 32 and len(got["binaural_direct_0_0"]) == 33

    # the two range checks, with their texts
    row, paths = data["reflection"][0][0], data["reflection"][1][0].copy()
    d_row, d_paths = data["diffraction"][0][0], data["diffraction"][1][0].copy()
    text29 = "Voices: triangle index 2^29 or above: the keys of the path kinds would collide"
    text28 = "Voices: a diffraction path's triangle index is 2^28 or above: its key would collide with the mixed paths' keys"
    paths[2]["triangle"] = 1 << 29
    assert plug.Voices(row, paths)["key"][2] == 1 << 29
    assert plug.Voices(row, paths, pathing=pathing[0])["key"][2] == 1 << 29, "pathing alone arms no check"
    for kind in KINDS[1:]:
        with pytest.raises(ValueError) as e:
            plug.Voices(row, paths, **{kind: (data[kind][0][0], data[kind][1][0])})
        assert str(e.value) == text29, kind
    paths[2]["triangle"] = (1 << 29) - 1
    d_paths[1]["triangle"] = 1 << 29
    with pytest.raises(ValueError) as e:
        plug.Voices(row, paths, diffraction=(d_row, d_paths), mixed=(data["mixed"][0][0], data["mixed"][1][0]))
    assert str(e.value) == text29
    d_paths[1]["triangle"] = 1 << 28
    second = data["second"][0][0], data["second"][1][0]
    assert plug.Voices(row, paths, diffraction=(d_row, d_paths), second=second)["key"][int(row["returned"]) + 1] == cap.DIFFRACTION_VOICE_TAG | ((1 << 30) + int(d_paths[1]["edge"]))
    with pytest.raises(ValueError) as e:
        plug.Voices(row, paths, diffraction=(d_row, d_paths), second=second, mixed=(data["mixed"][0][0], data["mixed"][1][0]))
    assert str(e.value) == text28
