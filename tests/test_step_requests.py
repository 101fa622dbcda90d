"""The traversal step's requests and direction signs, pinned bit for bit ("Fewer vector instructions
from arrival to request").  The step addresses its records by a scalar base and a 32-bit offset per lane and keeps the
signs of a ray's direction as three lane masks of the wave, made where a traversal starts and again when lanes take other
lanes' rays.  Where that goes wrong is small: a direction component of -0.0 or +0.0 (the compare is `inv < 0.0f`), a wave
whose lanes have unlike signs, a thief that keeps its old signs, a tree whose root is a leaf, a scene without a tree.
None may change a bit: hits and deterministic integer energy are compared with arrays recorded from the build BEFORE the
change (tests/golden/step_requests_*.npz, written once by tests/golden/make_golden_step_requests.py and never since)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_parity import make_ctx

pytestmark = pytest.mark.gpu
DET = 8   # FS_FLAG_DETERMINISTIC: integer deposits, the same energy however the frame is scheduled

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = {"starter_room": 4, "old_mine": 8}
DEGENERATE = ("one_triangle", "empty")
N_RAYS = 64
# per-ray search lengths (cm): both scenes are closed around the source, so the shortest ones miss and the longest hit
TMAX_LADDER = (10.0, 100.0, 300.0, 1000.0, 3000.0, 1e6)
RAY_KEYS = ("hit", "t_bits", "tri", "any_hit")


def golden_path(name):
    return os.path.join(GOLDEN_DIR, f"step_requests_{name}.npz")


def wave_of_rays(source):
    """64 rays from `source`, one wave: the six axis directions with their two zero components as +0.0 / -0.0 in all four
    ways (24), one zero component of either sign next to two components of every sign pair (24), the eight octant
    diagonals (8) and eight seeded diagonal rays of unlike magnitudes (8); search lengths from TMAX_LADDER, shuffled."""
    d = []
    for axis in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    v = [z1, z2]
                    v.insert(axis, s)
                    d.append(v)
    for axis in range(3):
        for z in (0.0, -0.0):
            for s1 in (1.0, -1.0):
                for s2 in (1.0, -1.0):
                    v = [s1, s2]
                    v.insert(axis, z)
                    d.append(v)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                d.append([sx, sy, sz])
    rng = np.random.default_rng(0x51E9)
    d = np.concatenate([np.asarray(d, np.float32), rng.normal(size=(8, 3)).astype(np.float32)])
    assert d.shape == (N_RAYS, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)   # (-0.0 / norm stays -0.0)
    o = np.tile(np.asarray(source, np.float32), (N_RAYS, 1))
    tmax = rng.permutation(np.tile(np.asarray(TMAX_LADDER, np.float32), 11)[:N_RAYS])
    return o, d, tmax


def trace(ctx, o, d, tmax):
    hit, t, tri, _ = ctx.trace_rays(o, d, tmax)
    any_hit = ctx.trace_rays(o, d, tmax, any_hit=True)[0]
    return {"hit": hit.astype(np.uint8), "t_bits": t.view(np.uint32).copy(), "tri": tri.astype(np.int32),
            "any_hit": any_hit.astype(np.uint8)}


def frame_params(pkg):
    return pkg.default_params(num_rays=16384, depth=8, seed=0x51E9, flags=DET)


def record(pkg, sc):
    """what a golden file holds (also called by tests/golden/make_golden_step_requests.py)"""
    ctx, src = make_ctx(pkg, sc)
    out = trace(ctx, *wave_of_rays(sc.source))
    out["energy"] = ctx.compute_energy_response(src, frame_params(pkg)).copy()
    ctx.close()
    return out


def degenerate_scene(pkg, name):
    """one_triangle: the tree's root is a leaf (a 1 m triangle 20 m down the +x axis); empty: no tree at all"""
    box = pkg.scenes.shoebox(2)
    tri = np.array([[[2000.0, -50.0, -50.0], [2000.0, 50.0, -50.0], [2000.0, 0.0, 50.0]]], np.float32)
    if name == "empty":
        tri = np.zeros((0, 3, 3), np.float32)
    return SimpleNamespace(name=name, num_bands=2, triangles=tri, material_ids=np.zeros(len(tri), np.uint16),
                           absorption=box.absorption, source=np.array([0.0, 0.0, 0.0], np.float32),
                           listener=np.array([0.0, 300.0, 0.0], np.float32))


def check_fractions(name, g):
    """an all-miss (or all-hit) recording cannot pass for agreement"""
    for key in ("hit", "any_hit"):
        frac = float(g[key].mean())
        print(f"{name}: {key} fraction {frac:.3f}")
        assert 0.10 <= frac <= 0.90, (name, key, frac)


@pytest.fixture(scope="module")
def golden():
    return {name: dict(np.load(golden_path(name))) for name in list(SCENES) + list(DEGENERATE)}


@pytest.mark.parametrize("name", list(SCENES))
def test_golden_recording_has_hits_and_misses(golden, name):
    g = golden[name]
    assert g["hit"].shape == (N_RAYS,) and g["any_hit"].shape == (N_RAYS,)
    check_fractions(name, g)
    assert g["energy"].any()


@pytest.mark.parametrize("name", list(SCENES))
def test_one_wave_of_signed_zero_and_mixed_sign_rays(pkg, scene_factory, golden, monkeypatch, name):
    """trace_rays: the lane-private traversal (trav_run), closest hit and any hit, one wave with every sign pattern"""
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    sc = scene_factory(name, SCENES[name])
    ctx, _ = make_ctx(pkg, sc)
    got = trace(ctx, *wave_of_rays(sc.source))
    ctx.close()
    for key in RAY_KEYS:
        assert np.array_equal(got[key], golden[name][key]), (name, key)


@pytest.mark.parametrize("name,cap", [("starter_room", None), ("old_mine", None), ("old_mine", 12)])
def test_frame_energy_with_stealing_among_unlike_signs(pkg, scene_factory, golden, monkeypatch, name, cap):
    """a 16 384-ray, depth-8 deterministic frame: the waves' lanes take each other's rays (trav_shared) all the time, and
    diffuse rays of one wave point everywhere.  cap = 12 on the mine: registers shift around the deep store's code."""
    if cap is None:
        monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    else:
        monkeypatch.setenv("FS_STACK_ROWS_CAP", str(cap))
    sc = scene_factory(name, SCENES[name])
    ctx, src = make_ctx(pkg, sc)
    e = ctx.compute_energy_response(src, frame_params(pkg)).copy()
    ctx.close()
    assert e.any()
    assert np.array_equal(e, golden[name]["energy"]), (name, cap)


@pytest.mark.parametrize("name", list(SCENES))
def test_pipelined_frame_energy_equals_plain(pkg, scene_factory, golden, monkeypatch, name):
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    sc = scene_factory(name, SCENES[name])
    ctx, src = make_ctx(pkg, sc)
    p = frame_params(pkg)
    e_plain = ctx.compute_energy_response(src, p).copy()
    ctx.set_pipelining(2)
    for _ in range(4):
        ctx.compute_energy_response_async(src, p)
    ctx.synchronize()
    e_piped = ctx.energy_buffer(src).copy()
    ctx.close()
    assert np.array_equal(e_plain, golden[name]["energy"]), name
    assert np.array_equal(e_piped, e_plain), name


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_trees(pkg, golden, monkeypatch, name):
    """a leaf root and no tree: rays that cannot hit anything find nothing, a frame deposits nothing but the direct
    sound, nothing faults"""
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    sc = degenerate_scene(pkg, name)
    ctx, src = make_ctx(pkg, sc)
    o, d, tmax = wave_of_rays(sc.source)
    away = d[:, 0] <= 0.0                       # the triangle lies on the +x axis: these cannot reach it
    got = trace(ctx, o, d, tmax)
    e = ctx.compute_energy_response(src, frame_params(pkg)).copy()
    if name == "one_triangle":                  # ... and the ray straight down the axis, long enough, does
        hit, t, tri, _ = ctx.trace_rays(o[:1], np.array([[1.0, 0.0, 0.0]], np.float32), 1e6)
        assert hit[0] and tri[0] == 0 and abs(float(t[0]) - 2000.0) < 0.01
    ctx.close()
    assert away.sum() >= 24
    assert not got["hit"][away].any() and not got["any_hit"][away].any()
    if name == "empty":
        assert not got["hit"].any() and not got["any_hit"].any()
    for key in RAY_KEYS:
        assert np.array_equal(got[key], golden[name][key]), (name, key)
    # The unoccluded direct connection source -> listener (3 m: bin 0) deposits in both scenes, in the recorded build
    # too; nothing else may.  Without a tree no walk finds a surface, so every other bin is zero; with the one
    # triangle the few walks that reach it must deposit exactly what the recorded build's did.
    assert np.array_equal(e, golden[name]["energy"]), (name, float(e.sum()))
    if name == "empty":
        assert not e[:, 1:].any(), (name, float(e[:, 1:].sum()))
