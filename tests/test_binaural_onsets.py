"""fs_binaural_render_process_batch with onsets on the HRIR set (fs_hrtf_set_onsets): the set's HRIRs are read as aligned and a
voice's HRIR is the aligned one — the nearest, or with a mesh the blend of three — delayed by the voice's own onset — the nearest's,
or the blend of the corners' (include/frequensee.h, "Onsets").

Nearest mode needs no model: a set with onsets must equal, bit for bit, the plain set of He taps the host delayed with
fs_hrtf_delay.  With a mesh the yardstick is hrtf_onsets_model's OnsetMeshModel, which the device must EQUAL (tobytes()); beside
it the same rule in float64 under a derived bound, what the feature is for as known answers, the spherical head's interaural delay
along a walk, and the state, batch and plumbing rules."""
import numpy as np
import pytest

from hrtf_mesh_model import OCTAHEDRON, SETS
from hrtf_onsets_model import OnsetMeshModel, OnsetModel, onset_bound
from test_binaural_interp import mesh_schedule
from test_binaural_render import assert_same, binaural_schedule, bound64, entry, make_set, one
from test_direct_paths import device_free_bytes
from test_direct_render import F32, FS
from test_direct_render import _close_contexts  # noqa: F401  (closes the contexts ctx_for caches when this module is done)
from test_direct_render import ctx_for, mix_model, noise, table_of
from test_reflection_render import POW2_FS, secs
from test_reverb_batch import noise_ir


def onset_set(pkg, name, H, rng, omax):
    """(dirs, hrir, tri, rows, onsets): a named set with random aligned HRIRs of H taps, triangulated by the library, its triangles
    shuffled and each rotated at random, and onsets uniform in [0, omax] with omax itself among them"""
    dirs = SETS[name]
    n = dirs.shape[0]
    tri = pkg.Context.hrtf_triangulate(dirs)
    tri = np.stack([np.roll(t, int(rng.integers(0, 3))) for t in tri[rng.permutation(tri.shape[0])]]).astype(np.int32)
    onsets = rng.uniform(0.0, omax, (n, 2)).astype(np.float32)
    onsets[int(rng.integers(0, n)), int(rng.integers(0, 2))] = omax
    return dirs, rng.uniform(-1.0, 1.0, (n, 2, H)).astype(np.float32), tri, pkg.Context.hrtf_mesh_rows(dirs, tri), onsets


def install(ctx, the_set, mesh=True, onsets=True, mesh_first=True):
    dirs, hrir, tri, rows, o = the_set
    ctx.hrtf_set(dirs, hrir)
    assert ctx.hrtf_onsets_info() == (False, 0)
    if mesh and mesh_first:
        ctx.hrtf_set_mesh(tri)
    if onsets:
        ctx.hrtf_set_onsets(o)
        assert ctx.hrtf_onsets_info() == (True, int(o.max()) + 1)
    if mesh and not mesh_first:
        ctx.hrtf_set_mesh(tri)
    assert ctx.hrtf_mesh_info() == (tri.shape[0] if mesh else 0) and ctx.hrtf_onsets_info()[0] == bool(onsets)


# ---- the restatement inside a float64 bound (no device) ---------------------------------------------------------------------------
def test_model_against_float64(pkg):
    """OnsetModel and OnsetMeshModel lie inside bound64 — test_binaural_render's, taken with He taps — plus onset_bound, derived
    in hrtf_onsets_model: the float64 side takes the index or the triangle from the fp32 rule and computes the weights, both
    blends, the delay, the fold and the tap loop in float64.  Every delayed HRIR the models fold is checked against
    fs_hrtf_delay's, bit for bit, on the way.  24 random cases, both modes, K <= 3 voices, the second callback
    ramping delays, gains and directions; the worst observed share of the bound is printed (DESIGN.md records it)."""
    rng = np.random.default_rng(0x0A5E)
    worst = own_share = 0.0
    for case in range(24):
        bands, taps, H, frame = int(rng.choice([1, 3, 8])), int(rng.choice([15, 63])), int(rng.choice([1, 7, 32])), 32
        K = int(rng.integers(1, 4))
        the_set = onset_set(pkg, ("octahedron", "fib16", "fib258")[case % 3], H, rng, float(rng.choice([0.75, 6.5, 31.25])))
        dirs, hrir, tri, rows, onsets = the_set
        table = pkg.Context.direct_band_kernels(FS, bands, taps)
        m = OnsetMeshModel(table, dirs, hrir, tri, rows, onsets, frame, K) if case % 2 else OnsetModel(table, dirs, hrir, onsets, frame, K)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            entries = [(k, float(rng.uniform(0.0, 300.0)) / FS, rng.uniform(0.0, 1.0, 8), float(rng.uniform(-1.0, 1.0)),
                        dirs[int(rng.integers(0, dirs.shape[0]))] if (case + k) % 4 == 0 else rng.normal(size=3)) for k in range(K)]
            extra = onset_bound(m, entries)
            for p in filter(None, m.match(entries)[0]):   # the model's delayed HRIRs are the library's, bit for bit (fs_hrtf_delay)
                for q in (p[4], p[8]):
                    for ear in range(2):
                        lib_hd = pkg.Context.hrtf_delay(np.asarray(m.hrir.inner[q, ear]), m.hrir.tau(q, ear)[0], m.H)
                        assert np.asarray(m.hrir[q, ear]).tobytes() == lib_hd.tobytes(), (case, q, ear)
            y, row, y64, w_loop, w_fold = m.process(blk, entries, want64=True)
        assert row == (K, 0, 0, 0)
        bound = bound64(taps, m.H, bands, K, w_loop, w_fold) + extra
        worst = max(worst, float(np.abs(y - y64).max() / bound))
        own_share = max(own_share, extra / bound)
    print(f"onset models vs float64: worst share of the bound {worst:.3f} (the onsets' own terms are at most {own_share:.3f} of it)")
    assert worst <= 1.0


# ---- GPU: bit equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fractional", "integer"])
@pytest.mark.parametrize("bands,frame,taps,H", [(1, 64, 1, 1), (3, 64, 15, 7), (1, 64, 15, 1), (3, 64, 1, 7)])
def test_nearest_mode_equals_the_host_delayed_set(pkg, bands, frame, taps, H, kind):
    """n = 6: the set with onsets against the plain set of He taps whose HRIRs the host delayed with fs_hrtf_delay, over the
    eight-callback script — bit for bit, and OnsetModel's bits too"""
    ctx = ctx_for(pkg, bands)
    rng = np.random.default_rng(3000 * bands + taps + 7 * H + (kind == "integer"))
    dirs, hrir = make_set(pkg, 6, H, rng)
    onsets = rng.uniform(0.0, 9.5, (6, 2)).astype(np.float32)
    if kind == "integer":
        onsets = np.floor(onsets)
    onsets[0, 0], onsets[5, 1] = 0.0, 9.0 if kind == "integer" else 9.5
    extra = int(onsets.max()) + 1
    plain = np.stack([np.stack([pkg.Context.hrtf_delay(hrir[j, ear], onsets[j, ear], H + extra) for ear in range(2)]) for j in range(6)])
    script = binaural_schedule(rng, dirs)
    blocks = [noise(rng, 1, frame)[0] for _ in script]

    def run(with_onsets):
        ctx.hrtf_set(dirs, hrir if with_onsets else plain)
        if with_onsets:
            ctx.hrtf_set_onsets(onsets)
        assert ctx.hrtf_onsets_info() == ((True, extra) if with_onsets else (False, 0))
        assert ctx.hrtf_info() == (6, H if with_onsets else H + extra)
        src = ctx.create_source()
        ctx.binaural_render_init(src, frame, taps, 3, 0.02)
        outs = [one(ctx, src, blk, entries) for blk, (entries, _) in zip(blocks, script)]
        ctx.destroy_source(src)
        return outs

    aligned, delayed = run(True), run(False)
    m = OnsetModel(table_of(pkg, ctx, taps), dirs, hrir, onsets, frame, 3)
    for cb, (got, want, blk, (entries, counts)) in enumerate(zip(aligned, delayed, blocks, script)):
        assert got[1] == counts
        assert_same(got, want, f"callback {cb + 1}: not the host-delayed set's")
        assert_same(got, m.process(blk, entries), f"callback {cb + 1}: not the model's")
    assert any(g[0].any() for g in aligned)
    ctx.hrtf_set(None, None)


# (bands, frame, taps, H, set, omax, callbacks): H = 1, 7 on both sets; He = 268 — the fold's 256-thread stride wraps in the fill and
# in the loop; He = FS_MAX_HRTF_TAPS exactly; Tc = 2001 + 47 - 1 = 2047 (three callbacks: the model's tap loop is the test's time);
# onsets all zero
MESH_SHAPES = [(1, 64, 1, 1, "octahedron", 9.5, 8), (3, 64, 15, 7, "fib16", 9.5, 8), (3, 64, 15, 1, "fib16", 4.0, 8),
               (1, 64, 1, 7, "octahedron", 6.25, 8), (3, 64, 15, 128, "fib16", 139.5, 8), (1, 64, 15, 372, "octahedron", 139.5, 8),
               (1, 64, 2001, 7, "fib16", 39.5, 3), (3, 64, 15, 7, "fib16", 0.0, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("bands,frame,taps,H,name,omax,callbacks", MESH_SHAPES)
def test_mesh_mode_is_bit_equal_to_the_model(pkg, bands, frame, taps, H, name, omax, callbacks):
    ctx = ctx_for(pkg, bands)
    rng = np.random.default_rng(4000 * bands + taps + 7 * H + int(8 * omax) + len(name))
    the_set = onset_set(pkg, name, H, rng, omax)
    install(ctx, the_set, mesh_first=bool(H % 2))
    He = H + int(F32(omax)) + 1
    assert He <= 512 and taps + He - 1 <= 2047
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, taps, 3, 0.02)
    m = OnsetMeshModel(table_of(pkg, ctx, taps), *the_set, frame, 3)
    assert m.H == He
    for cb, (entries, counts) in enumerate(mesh_schedule(rng, the_set[0])[:callbacks]):
        blk = noise(rng, 1, frame)[0]
        want = m.process(blk, entries)
        assert want[1] == counts, f"callback {cb + 1}: the yardstick's own counts"
        assert_same(one(ctx, src, blk, entries), want, f"callback {cb + 1}")
    ctx.destroy_source(src)
    ctx.hrtf_set(None, None)


@pytest.mark.gpu
def test_tc_limit_from_both_sides(pkg):
    """T = 2001, H = 7: onsets below 40 give He = 47 and Tc = 2047, which fs_binaural_render_init takes; an onset of 40 gives
    Tc = 2048: init refuses, and so does the callback for the source initialised before (the set has outgrown it)"""
    ctx = ctx_for(pkg, 1)
    rng = np.random.default_rng(2047)
    the_set = onset_set(pkg, "octahedron", 7, rng, 39.5)
    install(ctx, the_set)
    src = ctx.create_source()
    ctx.binaural_render_init(src, 64, 2001, 2, 0.01)
    blk = noise(rng, 1, 64)[0]
    entries = [entry(1, 10.0, np.ones(8), 1.0, (0.3, 0.2, 0.9))]
    assert one(ctx, src, blk, entries)[1] == (1, 1, 0, 0)
    more = the_set[4].copy()
    more[0, 0] = 40.0
    ctx.hrtf_set_onsets(more)
    assert ctx.hrtf_onsets_info() == (True, 41)
    with pytest.raises(pkg.FrequenSeeError):
        one(ctx, src, blk, entries)
    with pytest.raises(pkg.FrequenSeeError):
        ctx.binaural_render_init(src, 64, 2001, 2, 0.01)
    ctx.hrtf_set_onsets(the_set[4])
    assert one(ctx, src, blk, entries)[1] == (1, 1, 0, 0)   # (the refused init left the set-up as it was)
    ctx.destroy_source(src)
    ctx.hrtf_set(None, None)


@pytest.mark.gpu
def test_a_set_direction_is_nearest_mode(pkg):
    """the octahedron, whose rows are exact: a voice at a set direction has weights exactly (1, 0, 0) up to the corner's place,
    so its onset is the direction's own and the output equals nearest mode's with the same onsets by value"""
    rng = np.random.default_rng(66)
    frame, taps, H = 64, 15, 7
    the_set = onset_set(pkg, "octahedron", H, rng, 9.5)
    ctx, plain = ctx_for(pkg, 3), pkg.Context(num_bands=3)
    install(ctx, the_set)
    install(plain, the_set, mesh=False)
    a, b = ctx.create_source(), plain.create_source()
    ctx.binaural_render_init(a, frame, taps, 6, 0.02)
    plain.binaural_render_init(b, frame, taps, 6, 0.02)
    g = rng.uniform(0, 1, 8).astype(np.float32)
    for cb in range(3):
        blk = noise(rng, 1, frame)[0]
        entries = [entry(k, 30.5 + k + cb, g, 0.7, OCTAHEDRON[(k + cb) % 6] * F32((0.5, 1.0, 4.0)[k % 3])) for k in range(6)]
        got, near = one(ctx, a, blk, entries), one(plain, b, blk, entries)
        assert got[1] == near[1] and np.array_equal(got[0], near[0]), f"callback {cb + 1}: not nearest mode's output"
    assert got[0].any()
    ctx.destroy_source(a)
    ctx.hrtf_set(None, None)
    plain.close()


# ---- GPU: what the feature is for --------------------------------------------------------------------------------------------------
def steady_response(ctx, src, frame, direction, delay_samples, fs):
    """the impulse response of one held voice: a callback on silence in which it arrives at `direction`, then an impulse"""
    entries = [(1, delay_samples / fs, np.ones(8, np.float32), 1.0, direction)]
    one(ctx, src, np.zeros(2 * frame, np.float32), entries)
    blk = np.zeros(2 * frame, np.float32)
    blk[0] = blk[1] = 1.0
    out, row = one(ctx, src, blk, entries)
    assert row == (1, 0, 0, 0)
    return out[0::2], out[1::2]


@pytest.mark.gpu
def test_two_onsets_blend_into_one_arrival(pkg):
    """the octahedron, H = 1, taps 1.0, one band (its kernel of T = 1 is exactly 1); the left ear's onsets are 3 at +x and 10 at +y,
    all others 0; a held voice at 20 samples from the normalised midpoint of +x and +y, whose weights are exactly a half each: an
    impulse arrives as 0.5, 0.5 at samples 20 + 6 and 20 + 7 — a delay of 6.5 — and its magnitude at fs / 14 is cos(pi / 14) =
    0.9749.  The same set installed as plain 11-tap deltas and blended — the behaviour without onsets, documented here — puts 0.5
    at 20 + 3 and 20 + 10: a comb whose null is at fs / 14"""
    ctx = ctx_for(pkg, 1, POW2_FS)
    frame = 64
    onsets = np.zeros((6, 2), np.float32)
    onsets[0, 0], onsets[2, 0] = 3.0, 10.0
    tri = pkg.Context.hrtf_triangulate(OCTAHEDRON)
    mid = (np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)).astype(np.float32)
    w14 = np.exp(-2j * np.pi * np.arange(frame) / 14.0)

    ctx.hrtf_set(OCTAHEDRON, np.ones((6, 2, 1), np.float32))
    ctx.hrtf_set_mesh(tri)
    ctx.hrtf_set_onsets(onsets)
    assert ctx.hrtf_onsets_info() == (True, 11)
    src = ctx.create_source()
    ctx.binaural_render_init(src, frame, 1, 2, 0.001)
    left, right = steady_response(ctx, src, frame, mid, 20.0, POW2_FS)
    want = np.zeros(frame, np.float32)
    want[26] = want[27] = 0.5
    assert np.array_equal(left, want), np.nonzero(left)
    assert np.array_equal(right, np.eye(1, frame, 20, dtype=np.float32)[0])
    aligned_mag = abs(np.sum(left[20:] * w14[:frame - 20]))
    assert aligned_mag >= 0.97 and abs(aligned_mag - np.cos(np.pi / 14.0)) <= 1e-6

    deltas = np.zeros((6, 2, 11), np.float32)
    deltas[:, :, 0] = 1.0
    deltas[0, 0], deltas[2, 0] = np.eye(1, 11, 3)[0], np.eye(1, 11, 10)[0]
    ctx.hrtf_set(OCTAHEDRON, deltas)
    ctx.hrtf_set_mesh(tri)
    ctx.binaural_render_init(src, frame, 1, 2, 0.001)
    left, right = steady_response(ctx, src, frame, mid, 20.0, POW2_FS)
    want = np.zeros(frame, np.float32)
    want[23] = want[30] = 0.5
    assert np.array_equal(left, want), np.nonzero(left)
    assert abs(np.sum(left[20:] * w14[:frame - 20])) <= 1e-6, "the time-domain blend's comb has its null at fs / 14"
    ctx.destroy_source(src)
    ctx.hrtf_set(None, None)


def lag_of(left, right):
    """the lag, in samples, of the cross-correlation peak of the two ears: positive where the left ear is later"""
    xc = np.correlate(left.astype(np.float64), right.astype(np.float64), "full")
    return int(np.argmax(xc)) - (right.shape[0] - 1)


def walk_lags(responses):
    lags = np.array([lag_of(l, r) for l, r in responses])
    return lags, np.abs(np.diff(lags))


@pytest.mark.gpu
@pytest.mark.parametrize("half", ["front", "rear"])
def test_spherical_head_delay_glides(pkg, half):
    """the spherical head at 64 directions through SetHrtf(interpolate=True, align=True): a source walks a half of the horizontal
    circle from the left ear's side to the right's in 1 degree steps — round the front, or round the back —, held at every step.
    The interaural delay — the lag of the cross-correlation peak of the two ears' steady impulse responses — never moves back, and
    no step exceeds the cap: the largest difference |o[a][ear] - o[b][ear]| between the onsets of two directions that share a mesh
    edge, over both ears, derived here from the set.  With align=False the blend cross-fades two arrivals, and the peak hops from
    one to the other by a whole neighbour difference: the same walk has a step of at least the median such difference of the set
    (a typical one; the cap is the largest), and more than the aligned walk's largest"""
    frame, H = 128, 64
    degrees = np.arange(-90, 91) if half == "front" else np.arange(270, 89, -1)
    azimuths = np.radians(degrees)
    aims = np.stack([np.cos(azimuths), np.sin(azimuths), np.zeros_like(azimuths)], 1).astype(np.float32)

    def walk(align):
        sub = pkg.AudioRayTracingSubsystem(num_bands=1)
        plug = pkg.FrequenSeeAudioBinauralPlugin(sub)
        plug.SetHrtf(directions=64, taps=H if not align else 32, interpolate=True, align=align)
        ctx = sub.ctx
        assert ctx.hrtf_onsets_info()[0] == align and ctx.hrtf_mesh_info() == 124
        srcs = [ctx.create_source() for _ in aims]
        for s in srcs:
            ctx.binaural_render_init(s, frame, 1, 1, 0.001)
        lists = [[(1, 0.0, np.ones(8, np.float32), 1.0, d)] for d in aims]
        # a source per step, all in one batch: the voices arrive on silence, then an impulse
        ctx.binaural_render_process_batch(srcs, np.zeros((len(srcs), 2 * frame), np.float32), lists)
        blk = np.zeros((len(srcs), 2 * frame), np.float32)
        blk[:, :2] = 1.0
        out, _ = ctx.binaural_render_process_batch(srcs, blk, lists)
        sub.Deinitialize()
        return walk_lags([(o[0::2], o[1::2]) for o in out])

    dirs, _, onsets = pkg.Context.hrtf_spherical_head_split(FS, 64, 32)
    tri = pkg.Context.hrtf_triangulate(dirs)
    o = onsets.astype(np.float64)
    neighbours = np.array([abs(o[t[i], ear] - o[t[(i + 1) % 3], ear]) for t in tri for i in range(3) for ear in range(2)])
    cap, typical = neighbours.max(), np.median(neighbours)
    lags, steps = walk(True)
    plain_lags, plain_steps = walk(False)
    print(f"interaural lag along the {half} walk: aligned {lags[0]} .. {lags[-1]}, largest step {steps.max()} (cap {cap:.2f}, median "
          f"neighbour difference {typical:.2f}); time-domain blend {plain_lags[0]} .. {plain_lags[-1]}, largest step {plain_steps.max()}")
    assert lags[0] < -20 and lags[-1] > 20, "the left ear is early on its own side and late on the other"
    assert np.all(np.diff(lags) >= 0), "the interaural delay moved back"
    assert steps.max() <= cap
    assert plain_steps.max() >= typical and plain_steps.max() > steps.max()


# ---- GPU: state ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_onsets_change_start_every_voice_and_refusals_change_nothing(pkg):
    """Voices are held through every call below.  After fs_hrtf_set_onsets (install, clear), fs_hrtf_set_mesh with onsets in
    force, fs_hrtf_set (which drops both) the next callback reports every voice as started and is, with the one after it, the
    output of a context that never saw the call: one set up in that state from the start, which heard the same blocks without a
    voice (the history is kept, the slots are freed).  The mesh and the onsets are installed in one order here and in the other
    there.  A refused call changes nothing: the voices go on, bit for bit"""
    cap = pkg._capi
    rng = np.random.default_rng(23)
    frame, taps, H, K = 64, 15, 7, 3
    the_set = onset_set(pkg, "fib16", H, rng, 9.5)
    dirs, hrir, tri, rows, onsets = the_set
    ctx = pkg.Context(num_bands=3)
    lib = ctx.lib
    assert lib.fs_hrtf_set_onsets(ctx.h, onsets.ctypes.data) == cap.ERR_INVALID_ARGUMENT, "no set in force"
    assert lib.fs_hrtf_set_onsets(None, None) == cap.ERR_INVALID_ARGUMENT and lib.fs_hrtf_onsets_info(None, None, None) == cap.ERR_INVALID_ARGUMENT
    assert lib.fs_hrtf_onsets_info(ctx.h, None, None) == cap.OK
    ctx.hrtf_set(dirs, hrir)
    a = ctx.create_source()
    ctx.binaural_render_init(a, frame, taps, 4, 0.05)   # (a ring with room for every He below)
    heard = []

    def entries_now():
        return [entry(k, rng.uniform(0, 300), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(K)]

    def callback(started, other=None):
        blk, entries = noise(rng, 1, frame)[0], entries_now()
        got = one(ctx, a, blk, entries)
        assert got[1] == (K, K if started else 0, 0, 0)
        if other is not None:
            assert_same(got, one(*other, blk, entries), "not a context's that never saw the call")
        heard.append(blk)
        return got

    def never(**state):
        """a context in `state` from the start that heard every block so far without a voice"""
        c = pkg.Context(num_bands=3)
        install(c, the_set, **state)
        s = c.create_source()
        c.binaural_render_init(s, frame, taps, 4, 0.05)
        for blk in heard:
            assert one(c, s, blk, [])[1] == (0, 0, 0, 0)
        return c, s

    def check(**state):
        other = never(**state)
        callback(True, other)
        callback(False, other)
        return other

    callback(True)
    callback(False)
    ctx.hrtf_set_onsets(onsets)   # install, nearest mode
    assert ctx.hrtf_onsets_info() == (True, 10) and ctx.hrtf_mesh_info() == 0
    other = check(mesh=False)
    refused = []
    for value in (np.nan, np.inf, -0.5, 505.0):   # 7 + 505 + 1 > 512
        bad = onsets.copy()
        bad[3, 1] = value
        refused.append(bad)
    for bad in refused:
        assert lib.fs_hrtf_set_onsets(ctx.h, bad.ctypes.data) == cap.ERR_INVALID_ARGUMENT
    assert ctx.hrtf_onsets_info() == (True, 10)
    callback(False, other)   # nothing started anew
    other[0].close()
    fits = onsets.copy()
    fits[3, 1] = 504.0   # He = 512 exactly is accepted (and cleared again below: this source's ring is not asked for it)
    ctx.hrtf_set_onsets(fits)
    assert ctx.hrtf_onsets_info() == (True, 505)
    ctx.hrtf_set_onsets(onsets)
    callback(True)
    ctx.hrtf_set_mesh(tri)   # the mesh behind the onsets: they stay
    assert ctx.hrtf_onsets_info() == (True, 10) and ctx.hrtf_mesh_info() == tri.shape[0]
    check(mesh_first=True)[0].close()   # (there: the mesh first)
    ctx.hrtf_set_onsets(None)   # clear: the mesh stays
    assert ctx.hrtf_onsets_info() == (False, 0) and ctx.hrtf_mesh_info() == tri.shape[0]
    check(onsets=False)[0].close()
    ctx.hrtf_set_onsets(onsets)   # the onsets behind the mesh
    check(mesh_first=False)[0].close()   # (there: the onsets first)
    ctx.hrtf_set_mesh(None)   # the mesh goes, the onsets stay
    assert ctx.hrtf_onsets_info() == (True, 10) and ctx.hrtf_mesh_info() == 0
    check(mesh=False)[0].close()
    ctx.hrtf_set_mesh(tri)
    ctx.hrtf_set(dirs, hrir)   # a set, new or not, drops both
    assert ctx.hrtf_onsets_info() == (False, 0) and ctx.hrtf_mesh_info() == 0 and ctx.hrtf_info() == (16, H)
    check(mesh=False, onsets=False)[0].close()
    ctx.hrtf_set_onsets(onsets)
    ctx.hrtf_set(None, None)
    assert ctx.hrtf_onsets_info() == (False, 0)
    ctx.close()


@pytest.mark.gpu
def test_a_source_initialised_before_is_refused_until_initialised_again(pkg):
    """max delay 936 samples, F = 64, T = 15, H = 7: D + Tc + 1 + F = 1022 fits the ring of 1024; with onsets up to 9.5 Tc grows by
    10 and it does not: the callback refuses the source, changing nothing, until fs_binaural_render_init sizes it anew — from
    where it is a fresh context's source"""
    rng = np.random.default_rng(29)
    frame, taps, H = 64, 15, 7
    the_set = onset_set(pkg, "octahedron", H, rng, 9.5)
    ctx, fresh = ctx_for(pkg, 3), pkg.Context(num_bands=3)
    ctx.hrtf_set(the_set[0], the_set[1])
    src, other = ctx.create_source(), fresh.create_source()
    ctx.binaural_render_init(src, frame, taps, 2, 936.0 / FS)
    entries = [entry(1, 100.0, rng.uniform(0, 1, 8), 0.8, (0.2, -0.7, 0.4))]
    blk = noise(rng, 1, frame)[0]
    assert one(ctx, src, blk, entries)[1] == (1, 1, 0, 0)
    ctx.hrtf_set_mesh(the_set[2])
    assert one(ctx, src, blk, entries)[1] == (1, 1, 0, 0), "Tc does not depend on the mesh"
    ctx.hrtf_set_onsets(the_set[4])
    for _ in range(2):
        with pytest.raises(pkg.FrequenSeeError):
            one(ctx, src, blk, entries)
    ctx.binaural_render_init(src, frame, taps, 2, 936.0 / FS)
    install(fresh, the_set)
    fresh.binaural_render_init(other, frame, taps, 2, 936.0 / FS)
    for cb in range(2):
        blk = noise(rng, 1, frame)[0]
        assert_same(one(ctx, src, blk, entries), one(fresh, other, blk, entries), f"callback {cb + 1} after the new init")
    ctx.destroy_source(src)
    ctx.hrtf_set(None, None)
    fresh.close()


@pytest.mark.gpu
def test_batch_single_and_permuted_agree(pkg):
    """sources of 1, 3 and 8 slots with 0, 1 and 5 entries (rotating) in one batch of stride 5, with a mesh and onsets"""
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(5)
    frame, taps, n = 320, 15, 3
    the_set = onset_set(pkg, "fib16", 7, rng, 9.5)
    install(ctx, the_set)
    V = [1, 3, 8]
    sets = [[ctx.create_source() for _ in range(n)] for _ in range(3)]   # one call | three calls | permuted order
    for group in sets:
        for s, v in zip(group, V):
            ctx.binaural_render_init(s, frame, taps, v, 0.02)
    models = [OnsetMeshModel(table_of(pkg, ctx, taps), *the_set, frame, v) for v in V]
    perm = [2, 0, 1]
    counts = [[0, 1, 5], [1, 5, 0], [5, 0, 1], [1, 1, 5]]
    for cb in range(4):
        blk = noise(rng, n, frame)
        lists = [[entry(50 + k, rng.uniform(0, 600), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(counts[cb][i])]
                 for i in range(n)]
        out, mix, rows = ctx.binaural_render_process_batch(sets[0], blk, lists, stride=5, want_mix=True)
        singles = [one(ctx, sets[1][i], blk[i], lists[i], stride=5) for i in range(n)]
        pout, pmix, prows = ctx.binaural_render_process_batch([sets[2][i] for i in perm], blk[perm], [lists[i] for i in perm], stride=5,
                                                              want_mix=True)
        for i in range(n):
            want = models[i].process(blk[i], lists[i])
            assert_same((out[i], tuple(int(x) for x in rows[i])), want, f"batch {cb} {i}")
            assert_same(singles[i], want, f"single {cb} {i}")
            j = perm.index(i)
            assert_same((pout[j], tuple(int(x) for x in prows[j])), want, f"permuted {cb} {i}")
        assert mix.tobytes() == mix_model(out).tobytes(), "mix is not the fp32 sum in list order"
        assert pmix.tobytes() == mix_model(pout).tobytes()
    for s in sum(sets, []):
        ctx.destroy_source(s)
    ctx.hrtf_set(None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,onsets", [(False, False), (True, False), (False, True), (True, True)])
def test_steady_state_allocates_nothing(pkg, mesh, onsets):
    ctx = pkg.Context(num_bands=3)
    rng = np.random.default_rng(43)
    install(ctx, onset_set(pkg, "fib258", 32, rng, 20.5), mesh=mesh, onsets=onsets)
    frame, taps, n = 64, 15, 40
    srcs = [ctx.create_source() for _ in range(n)]
    for s in srcs:
        ctx.binaural_render_init(s, frame, taps, 4, 0.01)
    blk = noise(rng, n, frame)
    lists = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.0)) for k in range(3)]] * n
    ctx.binaural_render_process_batch(srcs, blk, lists[:n], stride=4, want_mix=True)
    free0 = device_free_bytes()
    for cb in range(20):
        more = [[(k, 0.001 * (k + 1), np.ones(8, np.float32), 1.0, (1.0, 0.5, 0.1 * cb)) for k in range(cb % 2, 4)]] * n   # slots fill up and turn over
        ctx.binaural_render_process_batch(srcs, blk, more, stride=4, want_mix=True)
    ctx.binaural_render_process_batch(srcs[:7], blk[:7], lists[:7], stride=3)   # a smaller shape fits what is there
    assert device_free_bytes() >= free0
    ctx.close()


@pytest.mark.gpu
def test_release_and_reinit(pkg):
    ctx = ctx_for(pkg, 3)
    rng = np.random.default_rng(10)
    the_set = onset_set(pkg, "octahedron", 7, rng, 6.5)
    install(ctx, the_set)
    src = ctx.create_source()
    frame, taps, V = 64, 15, 3
    ctx.binaural_render_init(src, frame, taps, V, 0.02)
    g = rng.uniform(0, 1, (2, 8)).astype(np.float32)
    entries = [entry(1, 50.5, g[0], 1.0, (0.0, 1.0, 0.2)), entry(2, 300.0, g[1], -0.5, (1.0, -1.0, 0.0))]
    for _ in range(2):
        one(ctx, src, noise(rng, 1, frame)[0], entries)
    ctx.binaural_render_release(src)   # zero history, every slot free: the same keys fade in from silence
    m = OnsetMeshModel(table_of(pkg, ctx, taps), *the_set, frame, V)
    for cb in range(2):
        blk = noise(rng, 1, frame)[0]
        got = one(ctx, src, blk, entries)
        assert got[1] == (2, 2 if cb == 0 else 0, 0, 0)
        assert_same(got, m.process(blk, entries), f"after release, callback {cb + 1}")
    for frame, taps, V in ((320, 15, 1), (64, 63, 5)):   # another F, another T, another V — with voices held
        ctx.binaural_render_init(src, frame, taps, V, 0.02)
        m = OnsetMeshModel(table_of(pkg, ctx, taps), *the_set, frame, V)
        for cb in range(2):
            blk = noise(rng, 1, frame)[0]
            assert_same(one(ctx, src, blk, entries), m.process(blk, entries), f"{(frame, taps, V)} callback {cb + 1}")
    ctx.destroy_source(src)   # with voices held
    other = ctx.create_source()
    ctx.binaural_render_init(other, 64, 15, 2, 0.02)
    m = OnsetMeshModel(table_of(pkg, ctx, 15), *the_set, 64, 2)
    blk = noise(rng, 1, 64)[0]
    assert_same(one(ctx, other, blk, entries), m.process(blk, entries), "a new source after the destroy")
    ctx.destroy_source(other)
    ctx.hrtf_set(None, None)
    closing = pkg.Context(num_bands=1)   # fs_context_destroy with a set, a mesh, onsets, a source and held voices
    install(closing, the_set)
    s = closing.create_source()
    closing.binaural_render_init(s, 64, 15, 2, 0.02)
    one(closing, s, blk, entries)
    closing.close()


@pytest.mark.gpu
def test_the_four_callbacks_alternate(pkg):
    """one "audio callback" = a reverb batch of 2, a direct batch of 5, a reflection batch of 3 and a binaural batch of 4 with a
    mesh and onsets, three rounds on one context; each equals what it gives alone"""
    frame, taps = 256, 15
    rng = np.random.default_rng(78)
    irs = [noise_ir(rng, 48000) for _ in range(2)]
    the_set = onset_set(pkg, "fib16", 7, rng, 9.5)
    rev_blocks = [noise(rng, 2, frame) * F32(0.3) for _ in range(3)]
    dir_blocks = [noise(rng, 5, frame) for _ in range(3)]
    ref_blocks = [noise(rng, 3, frame) for _ in range(3)]
    bin_blocks = [noise(rng, 4, frame) for _ in range(3)]
    tg = [[(float(F32(rng.uniform(0, 400) / FS)), rng.uniform(0, 1, 8).astype(np.float32)) for _ in range(5)] for _ in range(3)]
    ref_lists = [[[(k, secs(rng.uniform(0, 400)), rng.uniform(0, 1, 8).astype(np.float32), rng.uniform(-1, 1, 2).astype(np.float32))
                   for k in range(2 + cb)] for _ in range(3)] for cb in range(3)]
    bin_lists = [[[entry(k, rng.uniform(0, 400), rng.uniform(0, 1, 8), rng.uniform(-1, 1), rng.normal(size=3)) for k in range(1 + cb)]
                  for _ in range(4)] for cb in range(3)]

    def run(reverb, direct, reflect, binaural):
        ctx = pkg.Context(num_bands=1)
        install(ctx, the_set)
        rs = [ctx.create_source() for _ in range(2)]
        ds = [ctx.create_source() for _ in range(5)]
        es = [ctx.create_source() for _ in range(3)]
        bs = [ctx.create_source() for _ in range(4)]
        for s, ir in zip(rs, irs):
            ctx.reverb_init(s, frame)
            ctx.set_impulse_response(s, ir)
        for s in ds:
            ctx.direct_render_init(s, frame, taps, 0.01)
        for s in es:
            ctx.reflection_render_init(s, frame, taps, 4, 0.01)
        for s in bs:
            ctx.binaural_render_init(s, frame, taps, 4, 0.01)
        outs = {"reverb": [], "direct": [], "reflect": [], "binaural": []}
        for cb in range(3):
            if reverb:
                outs["reverb"].append(ctx.reverb_process_batch(rs, rev_blocks[cb]).tobytes())
            if direct:
                outs["direct"].append(ctx.direct_render_process_batch(ds, dir_blocks[cb], tg[cb]).tobytes())
            if reflect:
                out, rows = ctx.reflection_render_process_batch(es, ref_blocks[cb], ref_lists[cb])
                outs["reflect"].append(out.tobytes() + rows.tobytes())
            if binaural:
                out, rows = ctx.binaural_render_process_batch(bs, bin_blocks[cb], bin_lists[cb])
                outs["binaural"].append(out.tobytes() + rows.tobytes())
        ctx.close()
        return outs

    together = run(True, True, True, True)
    assert together["reverb"] == run(True, False, False, False)["reverb"], "the reverb rows changed beside the other batches"
    assert together["direct"] == run(False, True, False, False)["direct"], "the direct rows changed beside the other batches"
    assert together["reflect"] == run(False, False, True, False)["reflect"], "the reflection rows changed beside the other batches"
    assert together["binaural"] == run(False, False, False, True)["binaural"], "the binaural rows changed beside the other batches"
