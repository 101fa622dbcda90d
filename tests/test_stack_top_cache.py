"""The traversal's LDS stack, pinned bit for bit.  Written for the experiment that kept the stack's top row(s) in registers
("The stack top in a register": measured, slower, not kept), these tests hold for any change to the
step's pops, pushes, deep-store refill or work sharing.  The places where such a change goes wrong are small — a pop
right behind a push, two pops in one step, the empty stack, a donated only entry, the deep store's refill, an any-hit
query cut short — and none of them may change a bit: closest hits, any hits and the integer energy sums of seeded
queries are compared with arrays recorded from the build BEFORE the experiment (tests/golden/stack_top_*.npz, written
once by tests/golden/make_golden_stack_top.py and never since)."""
import os

import numpy as np
import pytest

from test_gpu_parity import make_ctx

pytestmark = pytest.mark.gpu
DET = 8   # FS_FLAG_DETERMINISTIC: integer deposits, the same energy however the frame is scheduled

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = {"starter_room": 4, "old_mine": 8}
N_RAYS = 4096
ANY_TMAX = 3000.0
KEYS = ("hit", "t_bits", "tri", "any_hit", "energy")


def golden_path(name):
    return os.path.join(GOLDEN_DIR, f"stack_top_{name}_rays_and_energy.npz")


def golden_rays(sc, n=N_RAYS):
    """origins = the source + N(0, 5 m) (scene units are cm), unit directions"""
    rng = np.random.default_rng(0x570C)
    o = np.tile(np.asarray(sc.source, np.float32), (n, 1)) + rng.normal(scale=500.0, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


def trace(ctx, o, d):
    hit, t, tri, _ = ctx.trace_rays(o, d, 1e6)
    any_hit = ctx.trace_rays(o, d, ANY_TMAX, any_hit=True)[0]
    return {"hit": hit.astype(np.uint8), "t_bits": t.view(np.uint32).copy(), "tri": tri.astype(np.int32),
            "any_hit": any_hit.astype(np.uint8)}


def record(pkg, sc):
    """what the golden file holds (also called by tests/golden/make_golden_stack_top.py)"""
    ctx, src = make_ctx(pkg, sc)
    out = trace(ctx, *golden_rays(sc))
    p = pkg.default_params(num_rays=16384, depth=8, seed=0x570C, flags=DET)
    out["energy"] = ctx.compute_energy_response(src, p).copy()
    ctx.close()
    return out


@pytest.fixture(scope="module")
def golden():
    return {name: dict(np.load(golden_path(name))) for name in SCENES}


@pytest.mark.parametrize("name", list(SCENES))
def test_golden_recording_has_hits_and_misses(golden, name):
    """an all-miss (or all-hit) recording cannot pass for agreement"""
    g = golden[name]
    assert g["hit"].shape == (N_RAYS,) and g["any_hit"].shape == (N_RAYS,)
    for key in ("hit", "any_hit"):
        frac = float(g[key].mean())
        print(f"{name}: {key} fraction {frac:.3f}")
        assert 0.10 <= frac <= 0.90, (name, key, frac)
    assert g["energy"].any()


@pytest.mark.parametrize("name,cap", [("starter_room", None), ("old_mine", None), ("old_mine", 12)])
def test_bit_exact_against_the_recorded_build(pkg, scene_factory, golden, monkeypatch, name, cap):
    """cap = 12 on the mine: the deep store works all the time, trav_maintain moves rows every few steps"""
    if cap is None:
        monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    else:
        monkeypatch.setenv("FS_STACK_ROWS_CAP", str(cap))
    sc = scene_factory(name, SCENES[name])
    got = record(pkg, sc)
    for key in KEYS:
        assert np.array_equal(got[key], golden[name][key]), (name, cap, key)


@pytest.mark.parametrize("name", list(SCENES))
def test_one_wave_with_48_lanes_idle_from_the_first_step(pkg, scene_factory, golden, monkeypatch, name):
    """64 rays, one wave: 48 start outside the scene's bounds and point away (they finish at the root), the other 16 are
    the first 16 golden rays and must give rows 0 - 15 of the golden arrays.  (trace_rays runs the lane-private traversal,
    trav_run: the wave's idle lanes ride along; donation itself — trav_shared — is covered by the energy frames.)"""
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    sc = scene_factory(name, SCENES[name])
    o16, d16 = (a[:16] for a in golden_rays(sc))
    lo, hi = sc.triangles.min(axis=(0, 1)), sc.triangles.max(axis=(0, 1))
    rng = np.random.default_rng(48)
    d48 = np.abs(rng.normal(size=(48, 3))).astype(np.float32) + np.float32(0.1)   # every component away from the box
    d48 /= np.linalg.norm(d48, axis=1, keepdims=True)
    o48 = (hi + (hi - lo) * rng.uniform(0.1, 1.0, size=(48, 3))).astype(np.float32)
    # interleaved, so that idle and busy lanes alternate within the wave
    order = rng.permutation(64)
    o = np.concatenate([o16, o48])[order]
    d = np.concatenate([d16, d48])[order]
    back = np.argsort(order)
    ctx, _ = make_ctx(pkg, sc)
    got = {k: v[back] for k, v in trace(ctx, o, d).items()}
    ctx.close()
    assert not got["hit"][16:].any() and not got["any_hit"][16:].any()
    for key in ("hit", "t_bits", "tri", "any_hit"):
        assert np.array_equal(got[key][:16], golden[name][key][:16]), (name, key)


def test_pipelined_frames_equal_plain_ones(pkg, scene_factory, monkeypatch):
    """65 536 rays: the wide flavour of the frame kernel; 262 144 rays: the 128-VGPR flavour (the pattern of
    test_bounded_lds_stack_spills_to_the_deep_store, at the default cap only)"""
    monkeypatch.delenv("FS_STACK_ROWS_CAP", raising=False)
    sc = scene_factory("old_mine", 8)
    ctx, src = make_ctx(pkg, sc)
    p = pkg.default_params(num_rays=65536, depth=8, seed=4242, flags=DET)
    pbig = pkg.default_params(num_rays=262144, depth=8, seed=4244, flags=DET)
    e_plain = ctx.compute_energy_response(src, p).copy()
    e_big_plain = ctx.compute_energy_response(src, pbig).copy()
    ctx.set_pipelining(2)
    for _ in range(4):
        ctx.compute_energy_response_async(src, p)
    ctx.synchronize()
    e_piped = ctx.energy_buffer(src).copy()
    for _ in range(3):
        ctx.compute_energy_response_async(src, pbig)
    ctx.synchronize()
    e_big_piped = ctx.energy_buffer(src).copy()
    ctx.close()
    assert e_plain.any() and e_big_plain.any()
    assert np.array_equal(e_plain, e_piped)
    assert np.array_equal(e_big_plain, e_big_piped)
