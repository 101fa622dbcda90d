"""fs_source_set_order_window on the GPU: a source's traced frames deposit only the contributions whose ORDER — the number of the
path's nodes that a walk step's hit made — lies in [min_order, max_order].

The yardstick is the float64 model of tests/restate_walk.py: windowed(fr, lo, hi) of tests/test_order_window_cpu.py filters the pairs a
model frame keeps.  The acceptance rule is tests/test_gpu_restatement.py's with its own numbers (ENERGY_RTOL / mode_rtol, count x 2^-41
in deterministic mode, at most |Fr| bad bins) and one change: a flagged contribution whose hit count the library and the model disagree
on can add a deposit to the window or take one away, so the cap |Fr| gain / pairs applies to |R| and not to R > 0 alone.

Frames: 1 024 pairs, depth 4, roulette on, seed 101, 4 bands, walls cut 1 x 1 and 8 x 8; rw.LISTENER is behind the slab (no path of
order 0), LISTENER2 is in view of the source.  What the model counts in them is asserted by tests/test_order_window_cpu.py and, where a
case depends on it, here before the GPU is used.

Measured on an MI355X: end-to-end 0 (behind the slab) and 2 (in view) flagged pairs, deposits equal to the model's or one more, at
most one bad bin, largest relative difference of a good entry 1.2e-6; uniform and balance 6 flagged of 16 919, 4 deposits more than the
model's unflagged ones in [1, inf) and [3, inf), at most two bad bins, 2.6e-4 / 3.3e-4; [0, 0] exactly 1 047 deposits in bin 2; lobes
[2, inf) 604 / 604 deposits; depth 0 [3, inf): 407 flagged of 22 623, 14 856 deposits against 14 555, 32 bad bins.
"""
import ctypes as C

import numpy as np
import pytest

import restate_walk as rw
from test_directivity import OBLIQUE, cardioid
from test_gpu_restatement import DET, GAIN, SEED, context
from test_independent_restatement import ENERGY_RTOL, LOBES, MODES, UNBOUNDED_SEED, mode_frame, mode_rtol
from test_order_window_cpu import LISTENER2, UNBOUNDED, deposits_by_order, differing, frame_of, windowed
from test_room_parameters import ROOM, check_source

pytestmark = pytest.mark.gpu

PAIRS = 1024
TAG = "order_window"      # contexts of this module's own (the listener moves)


def ctx_for(pkg, cut, listener, **kw):
    ctx, _ = context(pkg, cut, tag=TAG, **kw)
    ctx.set_listener(listener)
    return ctx


def params(pkg, depth=4, flags=0, gain=GAIN, pairs=PAIRS, seed=SEED):
    return pkg.default_params(num_rays=2 * pairs, depth=depth, seed=seed, russian_roulette=1, flags=flags, energy_gain=gain)


def trace(pkg, ctx, lo, hi=None, table=None, **kw):
    """one frame of a new source with the window (and table) -> (histogram, stats)"""
    s = ctx.create_source(rw.SOURCE)
    ctx.set_source_order_window(s, lo, hi)
    if table is not None:
        ctx.set_source_orientation(s, OBLIQUE)
        ctx.set_source_directivity(s, table)
    ctx.reset_stats()
    G = ctx.compute_energy_response(s, params(pkg, **kw)).astype(np.float64)
    st = ctx.stats()
    ctx.destroy_source(s)
    return G, st


def check_window(pkg, ctx, fr, lo, hi, what, depth=4, flags=0, gain=GAIN, rtol=ENERGY_RTOL, pairs=PAIRS, seed=SEED):
    W = windowed(fr, lo, hi)
    nfr = W.flagged
    G, st = trace(pkg, ctx, lo, hi, depth=depth, flags=flags, gain=gain, pairs=pairs, seed=seed)
    assert st["segments"] == st["planned_segments"] == W.steps, what        # as without a window
    assert st["connections_tested"] == W.connections, what
    assert abs(st["deposits"] - W.deposits) <= nfr, (what, st["deposits"], W.deposits, nfr)
    H = np.asarray(W.H, np.float64) * (gain / GAIN)
    allow = rtol * H + 1e-30
    if flags & DET:
        allow = allow + np.asarray(W.count, np.float64)[None, :] * 2.0 ** -41
    R = G - H
    bad = np.abs(R) > allow
    ok = ~bad & (H > 0.0)
    worst = float((np.abs(R)[ok] / H[ok]).max()) if ok.any() else 0.0
    print(f"{what} window [{lo}, {hi}]: flagged {nfr} deposits {st['deposits']} / {W.deposits} bad bins {int(bad.any(axis=0).sum())} "
          f"worst relative difference {worst:.3e}")
    assert bad.any(axis=0).sum() <= nfr, (what, np.flatnonzero(bad.any(axis=0)))
    cap = nfr * gain * 1.0 / pairs * (1.0 + 1e-5)
    assert (np.abs(R[bad]) <= cap).all(), (what, R[bad], cap)
    return G, st, W


# ---- 1. windows against the model, end-to-end ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("listener", [rw.LISTENER, LISTENER2], ids=["behind_the_slab", "in_view"])
def test_end_to_end_windows_against_the_model(pkg, listener):
    fr = frame_of(None, listener)
    assert len(fr.flagged) <= 0.02 * PAIRS
    # [4, inf) and [5, inf) are where an implementation that counts steps instead of hits fails
    assert differing(fr, 4) >= 8 and differing(fr, 5) >= 8
    assert max(deposits_by_order(fr)) == 8
    for cut in (1, 8):
        ctx = ctx_for(pkg, cut, listener)
        for lo, hi in ((0, 3), (4, None), (5, None), (1, 1), (4, 6)):
            G, _, W = check_window(pkg, ctx, fr, lo, hi, f"end-to-end cut {cut}")
            assert W.deposits > 0 and G.sum() > 0.0
        G, st = trace(pkg, ctx, 9)                   # depth 4: no path has more than 8 hits
        assert not G.any() and st["deposits"] == 0
        assert st["connections_tested"] == PAIRS and st["segments"] == fr.steps


# ---- 2. windows against the model, all prefixes and lobes ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uniform", "balance"])
def test_all_prefix_windows_against_the_model(pkg, mode):
    fr = frame_of(mode, LISTENER2)
    assert fr.flagged <= 0.02 * fr.connections
    direct = windowed(fr, 0, 0)
    assert np.flatnonzero(direct.count).tolist() == [2] and direct.deposits == 1047       # (0, 0) and (1, 0), (0, 1), ... over missed steps
    assert differing(fr, 3) >= 8
    for cut in (1, 8):
        ctx = ctx_for(pkg, cut, LISTENER2)
        for lo, hi in ((0, 0), (1, None), (3, None), (0, 2)):
            G, _, _ = check_window(pkg, ctx, fr, lo, hi, f"{mode} cut {cut}", flags=MODES[mode][0], rtol=mode_rtol(mode))
            if (lo, hi) == (0, 0):
                assert np.flatnonzero(G.any(axis=0)).tolist() == [2]


def test_lobe_window_against_the_model(pkg):
    fr = frame_of("lobes", rw.LISTENER)
    assert len(fr.flagged) <= 0.02 * PAIRS and windowed(fr, 2).deposits > PAIRS // 10
    for cut in (1, 8):
        ctx = ctx_for(pkg, cut, rw.LISTENER, lobes=True)
        check_window(pkg, ctx, fr, 2, None, f"lobes cut {cut}", flags=LOBES, rtol=mode_rtol("lobes"))


# ---- 3. off is off ----------------------------------------------------------------------------------------------------------------------
def test_default_window_is_the_plain_route(pkg):
    p = params(pkg, flags=DET, gain=1e6)
    ctx = ctx_for(pkg, 8, LISTENER2)
    a, b = ctx.create_source(rw.SOURCE), ctx.create_source(rw.SOURCE)
    ctx.set_source_order_window(a, 4, None)
    windowed_bits = ctx.compute_energy_response(a, p).copy()
    ctx.set_source_order_window(a, 0, None)
    assert ctx.source_order_window(a) == (0, None)
    got, want = ctx.compute_energy_response(a, p).copy(), ctx.compute_energy_response(b, p).copy()
    assert np.array_equal(got, want) and not np.array_equal(windowed_bits, want)
    ctx.destroy_source(a); ctx.destroy_source(b)

    def held(touch):   # a context of its own: the pipeline counters run since its creation
        sc = rw.make_test_scene()
        tri, mat = sc.triangles(8)
        c = pkg.Context(num_bands=4)
        c.set_scene(np.asarray(tri, np.float32), np.asarray(mat, np.uint16), np.asarray(sc.absorption, np.float32))
        c.set_listener(LISTENER2)
        c.set_pipelining(1)
        s = c.create_source(rw.SOURCE)
        if touch:
            c.set_source_order_window(s, 2, 5)
            c.set_source_order_window(s, 0, UNBOUNDED)
        for k in range(3):
            c.compute_energy_response_async(s, params(pkg, flags=DET, gain=1e6, seed=SEED + k))
        c.synchronize()
        out = c.energy_buffer(s).copy(), c.pipeline_counters()
        c.close()
        return out
    (e1, c1), (e0, c0) = held(True), held(False)
    assert np.array_equal(e1, e0)
    # the counters of what was launched and how; host_waits / host_wait_us are times, and whether a stream wait was enqueued or
    # skipped says whether the event had completed by then: only their sum is the schedule's
    for c in (c1, c0):
        c["stream_waits"] = c.pop("stream_waits_enqueued") + c.pop("stream_waits_skipped")
        c.pop("host_waits"); c.pop("host_wait_us")
    assert c1 == c0, (c1, c0)
    assert c0["fused_launches"] > 0          # the frames were held


# ---- 4. partition on the device -----------------------------------------------------------------------------------------------------------
def assert_partition(lo_part, hi_part, whole, what):
    """deterministic mode: each histogram is ONE rounding to float32 of an exact integer sum and the two parts' integers add up to
    the whole's, so |A + B - C| <= 2^-24 (A + B + C) = 2^-23 C per bin, summed in float64"""
    A, B, Cw = (np.asarray(x, np.float64) for x in (lo_part, hi_part, whole))
    assert (np.abs(A + B - Cw) <= 2.0 ** -23 * Cw).all(), what


@pytest.mark.parametrize("mode", [None, "uniform"], ids=["end_to_end", "uniform"])
def test_windows_partition_the_frame_on_the_device(pkg, mode):
    flags = DET | (MODES[mode][0] if mode else 0)
    ctx = ctx_for(pkg, 8, LISTENER2)
    whole, st = trace(pkg, ctx, 0, flags=flags, gain=1e6)
    assert whole.sum() > 0.0
    for k in (1, 3, 5):
        a, sa = trace(pkg, ctx, 0, k - 1, flags=flags, gain=1e6)
        b, sb = trace(pkg, ctx, k, flags=flags, gain=1e6)
        assert a.any() and b.any()
        assert_partition(a, b, whole, (mode, k))
        assert sa["deposits"] + sb["deposits"] == st["deposits"]
        for s in (sa, sb):
            assert (s["segments"], s["planned_segments"], s["connections_tested"]) == \
                   (st["segments"], st["planned_segments"], st["connections_tested"])


# ---- 5. routes ----------------------------------------------------------------------------------------------------------------------------
def test_routes_agree(pkg):
    p = params(pkg, flags=DET, gain=1e6)
    ctx = ctx_for(pkg, 8, LISTENER2)
    plain, win, both = (ctx.create_source(rw.SOURCE) for _ in range(3))
    ctx.set_source_order_window(win, 4, None)
    ctx.set_source_order_window(both, 4, None)
    ctx.set_source_orientation(both, OBLIQUE)
    ctx.set_source_directivity(both, np.ones((4, 7), np.float32))
    want_plain = ctx.compute_energy_response(plain, p).copy()
    want = ctx.compute_energy_response(win, p).copy()
    assert want.any() and not np.array_equal(want, want_plain)
    assert np.array_equal(ctx.compute_energy_response(both, p), want)      # an all-ones table changes no bit
    ctx.compute_energy_response_async(win, p)
    ctx.set_source_order_window(win, 0, 1)                                 # a set call never reaches an enqueued frame
    ctx.synchronize()
    assert np.array_equal(ctx.energy_buffer(win), want)
    ctx.set_source_order_window(win, 4, None)
    ctx.update_sources([win], p)
    assert np.array_equal(ctx.energy_buffer(win), want)
    for batch in (lambda: (ctx.compute_energy_response_batch_async([plain, win, both], p), ctx.synchronize()),
                  lambda: ctx.update_sources([plain, win, both], p)):
        batch()
        assert np.array_equal(ctx.energy_buffer(plain), want_plain)         # a plain source in a mixed batch: what it gets alone
        assert np.array_equal(ctx.energy_buffer(win), want)
        assert np.array_equal(ctx.energy_buffer(both), want)
    for s in (plain, win, both):
        ctx.destroy_source(s)
    # a pipelined context: the windowed frame drains the held ones
    pipe = ctx_for(pkg, 8, LISTENER2, pipelining=2)
    a, w = pipe.create_source(rw.SOURCE), pipe.create_source(rw.SOURCE)
    pipe.set_source_order_window(w, 4, None)
    pipe.compute_energy_response_async(a, p)
    pipe.compute_energy_response_async(w, p)
    pipe.compute_energy_response_async(a, params(pkg, flags=DET, gain=1e6, seed=SEED + 1))
    pipe.synchronize()
    assert np.array_equal(pipe.energy_buffer(w), want)
    pipe.compute_energy_response_async(a, p)
    pipe.synchronize()
    assert np.array_equal(pipe.energy_buffer(a), want_plain)
    pipe.destroy_source(a); pipe.destroy_source(w)


# ---- 6. window x directivity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "uniform"], ids=["end_to_end", "uniform"])
def test_window_and_directivity(pkg, mode):
    """directivity applies to what is deposited: directional [1, inf) = directional - directional [0, 0]"""
    flags = DET | (MODES[mode][0] if mode else 0)
    ctx = ctx_for(pkg, 8, LISTENER2)
    table = cardioid(4)
    whole, st = trace(pkg, ctx, 0, table=table, flags=flags, gain=1e6)
    direct, sd = trace(pkg, ctx, 0, 0, table=table, flags=flags, gain=1e6)
    rest, sr = trace(pkg, ctx, 1, table=table, flags=flags, gain=1e6)
    omni, _ = trace(pkg, ctx, 1, flags=flags, gain=1e6)
    assert direct.any() and rest.any() and not np.array_equal(rest, omni)
    assert_partition(direct, rest, whole, mode)
    assert sd["deposits"] + sr["deposits"] == st["deposits"]


# ---- 7. depth 0 -------------------------------------------------------------------------------------------------------------------------------
def test_unbounded_depth_window_against_the_model(pkg):
    fr = mode_frame("uniform", 0, True, UNBOUNDED_SEED, 256, keep_pairs=True)
    assert fr.flagged <= 0.02 * fr.connections and fr.most_combinations > 81
    W = windowed(fr, 3)
    assert 0 < W.deposits < fr.deposits
    for cut in (1, 8):
        ctx = ctx_for(pkg, cut, rw.LISTENER)
        check_window(pkg, ctx, fr, 3, None, f"uniform depth 0 cut {cut}", depth=0, flags=MODES["uniform"][0], rtol=mode_rtol("uniform"),
                     pairs=256, seed=UNBOUNDED_SEED)


# ---- 8. room parameters follow ----------------------------------------------------------------------------------------------------------------
def test_room_parameters_describe_the_windowed_histogram(pkg):
    flags = MODES["uniform"][0]
    ctx = ctx_for(pkg, 8, LISTENER2)
    s = ctx.create_source(rw.SOURCE)
    onset = []
    for lo in (0, 1):
        ctx.set_source_order_window(s, lo, None)
        ctx.compute_energy_response(s, params(pkg, flags=flags), want_host=False)
        ctx.reconstruct_impulse_response(s, params(pkg, flags=flags | ROOM))
        _, rec = check_source(ctx, s, f"window [{lo}, inf)")      # within 2 ulp of the float64 restatement of fs_get_energy_buffer
        onset.append(rec[:, 1])
    assert (onset[1] > onset[0]).all(), onset
    ctx.destroy_source(s)


# ---- 9. validation ----------------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_and_changes_nothing(pkg):
    ctx = ctx_for(pkg, 1, rw.LISTENER)
    s = ctx.create_source(rw.SOURCE)
    assert ctx.source_order_window(s) == (0, None)
    ctx.set_source_order_window(s, 2, 5)
    assert ctx.source_order_window(s) == (2, 5)
    for lo, hi in ((-1, 3), (-1, None), (3, 2), (1, 0)):
        with pytest.raises(pkg.FrequenSeeError) as ei:
            ctx.set_source_order_window(s, lo, hi)
        assert ei.value.code == pkg._capi.ERR_INVALID_ARGUMENT
        assert ctx.source_order_window(s) == (2, 5)
    for call in (lambda: ctx.set_source_order_window(s + 17, 1, None), lambda: ctx.source_order_window(s + 17)):
        with pytest.raises(pkg.FrequenSeeError) as ei:
            call()
        assert ei.value.code == pkg._capi.ERR_BAD_HANDLE
    lo, hi = C.c_int32(-7), C.c_int32(-7)
    assert ctx.lib.fs_source_get_order_window(ctx.h, s, None, C.byref(hi)) == pkg._capi.ERR_INVALID_ARGUMENT
    assert ctx.lib.fs_source_get_order_window(ctx.h, s, C.byref(lo), None) == pkg._capi.ERR_INVALID_ARGUMENT
    assert (lo.value, hi.value) == (-7, -7)
    assert ctx.lib.fs_source_set_order_window(None, s, 0, 1) == pkg._capi.ERR_INVALID_ARGUMENT
    assert ctx.source_order_window(s) == (2, 5)
    ctx.set_source_order_window(s, 3, 3)                     # a single order, and the whole range, are accepted
    ctx.set_source_order_window(s, 0, UNBOUNDED)
    assert ctx.source_order_window(s) == (0, None)
    ctx.set_source_order_window(s, 1, None)
    ctx.destroy_source(s)
    s2 = ctx.create_source(rw.SOURCE)                        # a re-created handle starts at the default
    assert s2 == s and ctx.source_order_window(s2) == (0, None)
    ctx.destroy_source(s2)
