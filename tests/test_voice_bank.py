"""The voice bank that fs_reflection_render_process_batch and fs_binaural_render_process_batch share: what the two callbacks must
do alike, whoever drives them — the text and the order of their refusals, and the binaural renderer on the H = 1 set of ones
equalling the reflection renderer as a batch of sources with different slot counts (the single-source identity is
test_binaural_render.test_ones_set_is_the_reflection_renderer).  The yardsticks are the two renderers' own restatements.
"""
import ctypes as C

import numpy as np
import pytest

import test_binaural_render as br
import test_reflection_render as rr
from test_direct_render import FS, mix_model, noise, table_of

INVALID, BAD_HANDLE = "ERR_INVALID_ARGUMENT", "ERR_BAD_HANDLE"

NO_SET_CALL = "fs_binaural_render_process_batch: no HRIR set in force (fs_hrtf_set)"
NO_SET_INIT = "fs_binaural_render_init: no HRIR set in force (fs_hrtf_set)"
OUTGROWN = "the HRIR set in force has outgrown this source's history: call fs_binaural_render_init again"
COUNT = "count out of range (1 .. FS_MAX_REFLECTION_RENDER_BATCH)"
STRIDE = "stride out of range (1 .. FS_MAX_REFLECTION_VOICES)"
VOICE_COUNT = "a voice count outside 0 .. stride"
KEY_TWICE = "a key appears twice in one row"
DELAY = "a voice's delay is negative, not finite or beyond the source's max delay"
BAND_GAIN = "a voice's band gain is negative or not finite"
CHANNEL_GAIN = "a voice's channel gain is not finite"
GAIN = "a voice's gain is not finite"
DIRECTION = "a voice's direction is not finite or is the zero vector"
SOURCE_TWICE = "a source appears twice in the batch"
ONE_SHAPE = "the sources of a batch share one frame size and one tap count"
HANDLE = "bad source handle"
INIT_RANGES = "fs_%s_render_init: frame size outside 16 .. 16384, taps even or outside 1 .. 2047, voices outside 1 .. 32, or a bad max delay"
INIT_RING = {"reflection": "fs_reflection_render_init: max delay + taps + 1 + frame size exceed 1 048 576 samples",
             "binaural": "fs_binaural_render_init: max delay + folded taps + 1 + frame size exceed 1 048 576 samples"}
INIT_FOLDED = "fs_binaural_render_init: taps + the set's taps - 1 exceed 2047"
NOT_INITIALISED = "fs_%s_render_init has not been called for this source"
SET_SIZE = "fs_hrtf_desc.struct_size mismatch"
SET_RANGES = "fs_hrtf_set: directions outside 1 .. 4096, taps outside 1 .. 512, or a NULL array"
SET_RATE = "fs_hrtf_set: the set's sample rate is not the context's"
SET_DIRECTION = "fs_hrtf_set: a direction is not finite or not a unit vector"
SET_TAP = "fs_hrtf_set: a tap is not finite"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["reflection", "binaural"])
def test_refusal_texts_and_their_order(pkg, which):
    """every refusal test_refusals_change_nothing provokes, with its return code and the exact fs_last_error text (None: the call
    returns before it has a context to report to, and the text stays what it was); then the cases in which two things are wrong at
    once, which name the one the header's order of validation meets first; then a good callback, which still equals the
    restatement: no refused call changed anything"""
    binaural = which == "binaural"
    cap = pkg._capi
    lib = cap.load()
    ctx = pkg.Context(num_bands=3)
    rng = np.random.default_rng(5)
    frame, taps = 64, 15
    dirs, hrir = br.make_set(pkg, 6, 7, rng)
    init = getattr(lib, f"fs_{which}_render_init")
    release = getattr(lib, f"fs_{which}_render_release")
    process = getattr(lib, f"fs_{which}_render_process_batch")
    py_init = getattr(ctx, f"{which}_render_init")
    py_process = getattr(ctx, f"{which}_render_process_batch")
    dtype = pkg.Context.BINAURAL_VOICE_DTYPE if binaural else pkg.Context.REFLECTION_VOICE_DTYPE
    last = lambda: lib.fs_last_error(ctx.h).decode()

    def refused(rc, code, text, what):
        before = refused.text
        assert rc == getattr(cap, code), f"{what}: returned {rc}"
        refused.text = last()
        assert refused.text == (before if text is None else text), f"{what}: {refused.text!r}"

    refused.text = last()
    if binaural:
        early = ctx.create_source()
        refused(init(ctx.h, early, frame, taps, 3, C.c_float(0.01)), INVALID, NO_SET_INIT, "init without a set")
        ctx.hrtf_set(dirs, hrir)
    srcs = [ctx.create_source() for _ in range(3)]
    for s, v in zip(srcs, (2, 3, 4)):
        py_init(s, frame, taps, v, 0.01)   # D = 480
    other_frame, other_taps, uninit, dead = (ctx.create_source() for _ in range(4))
    py_init(other_frame, 128, taps, 3, 0.01)
    py_init(other_taps, frame, 31, 3, 0.01)
    py_init(dead, frame, taps, 3, 0.01)
    (ctx.reflection_render_init if binaural else ctx.direct_render_init)(uninit, frame, taps, *((3, 0.01) if binaural else (0.01,)))
    ctx.destroy_source(dead)
    table = table_of(pkg, ctx, taps)
    models = [br.Model(table, dirs, hrir, frame, v) if binaural else rr.Model(table, frame, v) for v in (2, 3, 4)]
    gains = np.full(8, 0.5, np.float32)
    tail = (0.5, (0.0, 1.0, 0.5)) if binaural else ((0.5, 0.25),)   # what an entry carries beyond the delay and the band gains

    def good_call():
        blk = noise(rng, 3, frame)
        if binaural:
            lists = [[br.entry(k, rng.uniform(0, 400), gains, 0.5, rng.normal(size=3)) for k in range(2)] for _ in range(3)]
        else:
            lists = [[rr.entry(k, rng.uniform(0, 400), gains, (0.5, 0.25)) for k in range(2)] for _ in range(3)]
        out, rows = py_process(srcs, blk, lists)
        for i in range(3):
            rr.assert_same((out[i], tuple(int(x) for x in rows[i])), models[i].process(blk[i], lists[i]), f"source {i}")

    good_call()
    blk = noise(rng, 3, frame)
    sentinel = np.full((3, 2 * frame), 7.0, np.float32)
    out, mix = sentinel.copy(), sentinel[0].copy()
    rows = np.full((3, 4), 7, np.uint32)
    inf, nan = float("inf"), float("nan")
    base = np.zeros((3, 2), dtype=dtype)
    for i in range(3):
        for e in range(2):
            base[i, e] = (e, 0.001 * (i + e + 1), gains) + tail

    def call(sources=srcs, count=3, table=base, counts=(2, 2, 2), stride=2, blocks=blk, dest=out, mixed=None, voices=True, cnts=True, handles=True):
        arr = (C.c_int32 * len(sources))(*sources)
        t = np.ascontiguousarray(table)
        n = np.asarray(counts, np.int32)
        return process(ctx.h, arr if handles else None, count, blocks.ctypes.data if blocks is not None else None,
                       t.ctypes.data if voices else None, n.ctypes.data if cnts else None, stride,
                       dest.ctypes.data if dest is not None else None, mixed.ctypes.data if mixed is not None else None, rows.ctypes.data)

    def with_entries(*changes):
        """base with (row, entry, field, value[, index]) applied"""
        t = base.copy()
        for row, e, field, value, *index in changes:
            if index:
                t[row, e][field][index[0]] = value
            else:
                t[row, e][field] = value
        return t

    def with_entry(field, value, *index):
        return with_entries((1, 1, field, value) + index)

    # ---- one thing wrong at a time: test_refusals_change_nothing's list
    for counts in ((2, 3, 2), (2, -1, 2)):
        refused(call(counts=counts), INVALID, VOICE_COUNT, counts)
    wide = np.zeros((3, 33), dtype=dtype)
    for stride, table_ in ((0, base), (-1, base), (33, wide)):
        refused(call(stride=stride, table=table_, counts=(0, 0, 0)), INVALID, STRIDE, stride)
    refused(call(table=with_entry("key", 0)), INVALID, KEY_TWICE, "a key twice in one row")
    for v in (-0.001, nan, inf, 481.0 / FS):
        refused(call(table=with_entry("delay", v)), INVALID, DELAY, v)
    for v in (-0.5, nan, inf):
        refused(call(table=with_entry("band_gain", v, 1)), INVALID, BAND_GAIN, v)
    for v in (nan, inf, -inf):
        if binaural:
            refused(call(table=with_entry("gain", v)), INVALID, GAIN, v)
            for axis in range(3):
                refused(call(table=with_entry("direction", v, axis)), INVALID, DIRECTION, (v, axis))
        else:
            refused(call(table=with_entry("channel_gain", v, 1)), INVALID, CHANNEL_GAIN, v)
    if binaural:
        refused(call(table=with_entry("direction", (0.0, -0.0, 0.0))), INVALID, DIRECTION, "the zero vector")
    for count in (0, -1, 257):
        refused(call(count=count), INVALID, COUNT, count)
    refused(call(sources=[srcs[0], srcs[1], srcs[0]]), INVALID, SOURCE_TWICE, "a source twice")
    refused(call(sources=[srcs[0], other_frame, srcs[2]]), INVALID, ONE_SHAPE, "another frame size")
    refused(call(sources=[srcs[0], other_taps, srcs[2]]), INVALID, ONE_SHAPE, "another tap count")
    refused(call(sources=[srcs[0], uninit, srcs[2]]), INVALID, NOT_INITIALISED % which, "not initialised")
    refused(call(sources=[srcs[0], dead, srcs[2]]), BAD_HANDLE, HANDLE, "a destroyed source")
    refused(call(sources=[srcs[0], 12345, srcs[2]]), BAD_HANDLE, HANDLE, "no such source")
    refused(call(sources=[-1, srcs[1], srcs[2]]), BAD_HANDLE, HANDLE, "a negative handle")
    refused(call(handles=False), INVALID, None, "sources == NULL")
    refused(call(blocks=None), INVALID, None, "in == NULL")
    refused(call(voices=False), INVALID, None, "voices == NULL")
    refused(call(cnts=False), INVALID, None, "voice_counts == NULL")
    refused(call(dest=None), INVALID, None, "out == NULL && mix == NULL")
    if binaural:
        refused(call(table=with_entry("direction", nan, 0), mixed=mix), INVALID, DIRECTION, "with a mix")
    else:
        refused(call(table=with_entry("delay", nan), mixed=mix), INVALID, DELAY, "with a mix")
    if binaural:   # refused sets
        desc = cap.HrtfDesc(C.sizeof(cap.HrtfDesc), 6, 7, FS, dirs.ctypes.data, hrir.ctypes.data)

        def set_with(**kw):
            d = cap.HrtfDesc(desc.struct_size, desc.directions, desc.taps, desc.sample_rate, desc.dirs, desc.hrir)
            for k, v in kw.items():
                setattr(d, k, v)
            return lib.fs_hrtf_set(ctx.h, C.byref(d))

        long_dirs, nan_dirs, nan_hrir = dirs.copy(), dirs.copy(), hrir.copy()
        long_dirs[4] *= np.float32(1.001)   # squared length 1.002
        nan_dirs[5, 1] = nan
        nan_hrir[3, 1, 6] = inf
        wide_dirs, wide_hrir = np.tile(dirs[:1], (4097, 1)), np.zeros((4097, 2, 1), np.float32)
        long_hrir = np.zeros((6, 2, 513), np.float32)
        for kw, text in ((dict(struct_size=desc.struct_size - 4), SET_SIZE), (dict(directions=0), SET_RANGES), (dict(directions=-1), SET_RANGES),
                         (dict(taps=0), SET_RANGES), (dict(sample_rate=FS + 1), SET_RATE), (dict(dirs=None), SET_RANGES), (dict(hrir=None), SET_RANGES),
                         (dict(dirs=long_dirs.ctypes.data), SET_DIRECTION), (dict(dirs=nan_dirs.ctypes.data), SET_DIRECTION),
                         (dict(hrir=nan_hrir.ctypes.data), SET_TAP),
                         (dict(directions=4097, taps=1, dirs=wide_dirs.ctypes.data, hrir=wide_hrir.ctypes.data), SET_RANGES),
                         (dict(taps=513, hrir=long_hrir.ctypes.data), SET_RANGES)):
            refused(set_with(**kw), INVALID, text, kw)
        assert ctx.hrtf_info() == (6, 7)
    # init and release
    folded = [((frame, 2043, 3, 0.01), INIT_FOLDED)] if binaural else []   # (2043 + 7 - 1 = 2049 folded taps)
    for args, text in [((15, 15, 3, 0.01), INIT_RANGES % which), ((16385, 15, 3, 0.01), INIT_RANGES % which), ((frame, 16, 3, 0.01), INIT_RANGES % which),
                       ((frame, 0, 3, 0.01), INIT_RANGES % which), ((frame, 2049, 3, 0.01), INIT_RANGES % which)] + folded + \
                      [((frame, taps, 0, 0.01), INIT_RANGES % which), ((frame, taps, -1, 0.01), INIT_RANGES % which),
                       ((frame, taps, 33, 0.01), INIT_RANGES % which), ((frame, taps, 3, -0.01), INIT_RANGES % which),
                       ((frame, taps, 3, nan), INIT_RANGES % which), ((frame, taps, 3, inf), INIT_RANGES % which),
                       ((frame, taps, 3, 22.0), INIT_RING[which])]:
        refused(init(ctx.h, srcs[0], args[0], args[1], args[2], C.c_float(args[3])), INVALID, text, args)
    refused(init(ctx.h, 12345, frame, taps, 3, C.c_float(0.01)), BAD_HANDLE, HANDLE, "init of no such source")
    refused(release(ctx.h, 12345), BAD_HANDLE, HANDLE, "release of no such source")
    assert release(ctx.h, uninit) == cap.OK

    # ---- two things wrong at once: the first the order of validation meets is the one named
    refused(call(sources=[srcs[0], 12345, srcs[2]], table=with_entries((0, 1, "delay", nan))), INVALID, DELAY,
            "a bad delay in row 0, a bad handle in row 1")
    own_gain = ("gain", nan) if binaural else ("channel_gain", nan, 0)
    refused(call(table=with_entries((1, 1, "key", 0), (1, 1) + own_gain)), INVALID, KEY_TWICE, "a key twice and a non-finite gain in one row")
    if binaural:
        refused(call(table=with_entries((1, 1, "gain", inf), (1, 1, "direction", (0.0, 0.0, 0.0)))), INVALID, GAIN,
                "a non-finite gain and a zero direction in one entry")
    else:
        refused(call(table=with_entries((1, 1, "channel_gain", inf, 1), (2, 0, "delay", nan))), INVALID, CHANNEL_GAIN,
                "a non-finite channel gain, and a bad delay in the next row")
    refused(call(sources=[srcs[0], uninit, srcs[2]], counts=(3, 2, 2)), INVALID, VOICE_COUNT, "a count above stride in row 0, row 1 not initialised")
    assert np.array_equal(out, sentinel) and np.array_equal(mix, sentinel[0]) and np.all(rows == 7), "a refused call wrote"
    good_call()
    if binaural:
        # a set that outgrows an initialised source's ring, between the row's first checks and its voice count:
        # D + Tc + 1 + F = 480 + (15 + 512 - 1) + 1 + 64 > 1024
        ctx.hrtf_set(dirs, np.zeros((6, 2, 512), np.float32))
        refused(call(), INVALID, OUTGROWN, "an outgrown history")
        refused(call(sources=[srcs[0], 12345, srcs[2]], counts=(3, 2, 2)), INVALID, OUTGROWN, "outgrown in row 0 before its count and row 1's handle")
        refused(call(sources=[12345, srcs[1], srcs[2]]), BAD_HANDLE, HANDLE, "the handle before the outgrown history")
        # no set in force: the count and the stride come first, everything about a row after
        ctx.hrtf_set(None, None)
        assert ctx.hrtf_info() == (0, 0)
        refused(call(), INVALID, NO_SET_CALL, "a missing set")
        refused(init(ctx.h, uninit, frame, taps, 3, C.c_float(0.01)), INVALID, NO_SET_INIT, "init without a set")
        refused(call(count=0), INVALID, COUNT, "a count of 0 with no set")
        refused(call(stride=33, table=wide, counts=(0, 0, 0)), INVALID, STRIDE, "a stride of 33 with no set")
        refused(call(sources=[srcs[0], 12345, srcs[2]]), INVALID, NO_SET_CALL, "a bad handle with no set")
        ctx.hrtf_set(dirs, hrir)
        for m in models:
            m.set(dirs, hrir)   # (a set, even the same one, starts every voice anew on the kept history)
        assert np.array_equal(out, sentinel) and np.all(rows == 7), "a refused call wrote"
        good_call()
    ctx.close()


@pytest.mark.gpu
def test_ones_set_is_the_reflection_renderer_as_a_batch(pkg):
    """on the H = 1 set of ones the fold is the identity: three sources of 2, 3 and 4 slots in ONE fs_binaural_render_process_batch
    equal three such sources in one fs_reflection_render_process_batch with channel_gain = (gain, gain) — out, mix and rows, by
    value — over the eight-callback script, every source on a script of its own seed.  F = 320: the second tile has 64 live
    threads.  With 2 slots the script drops what finds no slot, with 4 it drops nothing: the rows differ between the sources"""
    bands, frame, taps = 3, 320, 15
    ctx = pkg.Context(num_bands=bands)
    ctx.hrtf_set(*br.ones_set())
    a, b = [ctx.create_source() for _ in range(3)], [ctx.create_source() for _ in range(3)]
    for sa, sb, v in zip(a, b, (2, 3, 4)):
        ctx.binaural_render_init(sa, frame, taps, v, 0.02)
        ctx.reflection_render_init(sb, frame, taps, v, 0.02)
    rng = np.random.default_rng(frame + taps)
    scripts = [rr.bank_schedule(np.random.default_rng(100 + i)) for i in range(3)]
    heard, row_sets = False, set()
    for cb in range(8):
        blk = noise(rng, 3, frame)
        lists = [scripts[i][cb][0] for i in range(3)]
        got, gmix, grows = ctx.binaural_render_process_batch(
            a, blk, [[(key, delay, gains, float(chan[0]), rng.normal(size=3)) for key, delay, gains, chan in lst] for lst in lists], want_mix=True)
        want, wmix, wrows = ctx.reflection_render_process_batch(
            b, blk, [[(key, delay, gains, (chan[0], chan[0])) for key, delay, gains, chan in lst] for lst in lists], want_mix=True)
        grows, wrows = [tuple(int(x) for x in r) for r in grows], [tuple(int(x) for x in r) for r in wrows]
        assert grows == wrows, f"callback {cb + 1}: rows"
        assert grows[1] == scripts[1][cb][1], f"callback {cb + 1}: the three-slot source follows the script's own counts"
        assert np.array_equal(got, want), f"callback {cb + 1}: out"
        assert np.array_equal(gmix, wmix), f"callback {cb + 1}: mix"
        assert gmix.tobytes() == mix_model(got).tobytes(), f"callback {cb + 1}: mix is the fp32 sum in list order"
        heard = heard or all(bool(got[i].any()) for i in range(3))
        row_sets.add(tuple(grows))
    assert heard and any(len(set(rows)) > 1 for rows in row_sets), "all three sources sounded, and not alike"
    ctx.close()
