// fs_capi_reverb.cpp — row f2, the reverb plugin's per-callback convolution (RVB.cpp:74-213) behind the C ABI: per-source set-up
// (fs_reverb_init / _set_engine / _set_crossfade / _release) and the audio callback.  There is ONE callback path, reverb_rows: a
// list of rows served by one set of launches (fs_reverb.hip, and fs_reverb_part.hip for the rows of the partitioned engine);
// fs_reverb_process is that list with one row.  The soundfield sources (fs_reverb_set_soundfield) have a callback of their own,
// soundfield_rows behind fs_reverb_soundfield_process_batch: the same per-source step, rows of C frame floats.
#include <cmath>

#include "fs_context.hpp"

namespace {

bool partitioned(const Source* s) { return s->rev_engine == FS_REVERB_ENGINE_PARTITIONED; }

// fs_reverb_set_crossfade: the callback's two IR copies, once the source has a reverb and a fade length — impulse responses for
// the direct engine, partition spectra for the partitioned one, which needs the one it convolves (h_to) without a fade too
// (both == false)
int alloc_fade(fs_context* ctx, Source* s, bool both) {
    const size_t bytes = partitioned(s) ? sizeof(float2) * ((size_t)s->part_K << s->part_n) * (size_t)s->part_sets
                                        : sizeof(float) * (size_t)ctx->num_samples;
    if (both && !s->d_fade_from) FS_HIP(ctx, hipMalloc((void**)&s->d_fade_from, bytes));
    if (!s->d_fade_to) FS_HIP(ctx, hipMalloc((void**)&s->d_fade_to, bytes));
    return FS_OK;
}

// the partitioned engine's twiddle table of N = 1 << n, in double on the host (as fs_apply_material_fd's); init time only
int part_twiddles(fs_context* ctx, int n) {
    if (ctx->d_rev_tw[n]) return FS_OK;
    const std::vector<float2> w = fsi::host_twiddles((size_t)1 << n);
    FS_HIP(ctx, hipMalloc((void**)&ctx->d_rev_tw[n], sizeof(float2) * w.size()));
    FS_HIP(ctx, hipMemcpy(ctx->d_rev_tw[n], w.data(), sizeof(float2) * w.size(), hipMemcpyHostToDevice));
    return FS_OK;
}

// the reverb callback's own blocks in its staging (fs_context::rev_stage): CallbackLayout::up; scratch[0] = the mono tails cur
// kRevLists: the three lists of the direct engine's rows, then those of the partitioned engine's
// kRevEarLists: the three lists of the rows with ears — zero bytes in a call without such a row, so every other offset stays
enum { kRevItems, kRevPartItems, kRevLists, kRevEarLists };

// the bytes of Source::d_ring: the direct engine's two history rings, or the partitioned engine's state block
size_t reverb_state_bytes(const Source* s) {
    if (!partitioned(s)) return sizeof(float) * 2 * kReverbRing;
    return sizeof(float2) * part_state_elems(s->part_n, s->part_K, !s->rev_sf, s->rev_sf ? s->part_sets : 1);
}

const char* const kNoFadeBuffers = "the crossfade's impulse-response buffers are missing: call fs_reverb_init again";
const char* const kSoundfieldSource = "the source is initialised with the soundfield (fs_reverb_set_soundfield): its callback is fs_reverb_soundfield_process_batch";

// One convolved source's step of a callback, under its ir_mu.  The callback has its own stream: it is never queued behind a traced
// frame on the compute stream.  The device-resident IR is written by reconstructs on the tail stream: read it behind the newest one
// and make the next one wait for this read — both through events, exchanged with the game thread under the source's ir_mu (the
// caller records ev_rev behind the launch that reads d_ir_mono, still under the lock).  With a crossfade (fs_reverb_set_crossfade)
// the callback convolves its own copies of the IR: it reads d_ir_mono only when a newer IR is there (ir_gen), once, into h_to —
// only then does it wait for the write and make the next one wait for it.  *takes: this callback is such a one.
// The step fills the row's descriptor: `it` of a direct row, `pit` of a partitioned one (the other is null).
// The partitioned engine convolves spectra of its own with or without a crossfade, so it takes in the same way in both cases: H_to
// from d_ir_mono, when a newer IR is there.
// A source with ears (fs_reverb_set_ears) is such a row whose spectra come from the band rows — written by the same launches as
// d_ir_mono, under the same events — and the context's ear carriers: it also takes when that set was replaced (ear_set_gen).
// A soundfield source (fs_reverb_set_soundfield) is the same with the soundfield carriers (sf_set_gen).
int reverb_step(fs_context* ctx, Source* s, hipStream_t rs, int frame, ReverbItem* it, ReverbPartItem* pit, bool* takes) {
    const bool part = pit != nullptr;
    const bool xfade = s->fade_len > 0;
    const bool own = xfade || part;   // the callback convolves copies of its own
    const bool tk = *takes = own && (!s->fade_primed || s->ir_gen != s->fade_gen || (s->rev_ears && s->ear_gen != ctx->ear_set_gen) ||
                                   (s->rev_sf && s->sf_gen != ctx->sf_set_gen));
    if ((!own || tk) && s->last_rec >= 0) {
        const int buf = s->last_rec;
        // (a finished reconstruct needs no barrier packet on the stream: S of them are most of a short batch)
        bool done = false;
        if (s->rec_recorded[buf] && !s->rec_batch[buf]) {
            done = hipEventQuery(s->ev_rec[buf]) == hipSuccess;
            if (!done) (void)hipGetLastError();   // hipErrorNotReady is not an error
        }
        if (!done) FS_HIP(ctx, stream_waits_for_rec(ctx, rs, s, buf));
    }
    if (tk) {
        float a = 0.0f;
        if (xfade && s->fade_primed) {   // a fade from what is heard now: h_to alone, or the mix at the last output sample of a running fade
            if (s->fading) a = (float)s->fade_pos / (float)s->fade_len;
            else std::swap(s->d_fade_from, s->d_fade_to);
            s->fading = true;
            s->fade_pos = 0;
        }
        if (part) { pit->take_from = (float2*)s->d_fade_from; pit->take_to = (float2*)s->d_fade_to; pit->take_ir = (s->rev_ears || s->rev_sf) ? s->d_ir_bands : s->d_ir_mono; pit->take_a = a; }
        else { it->take_from = s->d_fade_from; it->take_to = s->d_fade_to; it->take_ir = s->d_ir_mono; it->take_a = a; }
        s->fade_primed = true;
        s->fade_gen = s->ir_gen;
        s->ear_gen = ctx->ear_set_gen;
        s->sf_gen = ctx->sf_set_gen;
    }
    if (!own || tk) s->rev_recorded = true;
    if (part) {
        pit->active = 1;
        pit->state = (float2*)s->d_ring;
        pit->head = s->rev_head;
        pit->slot = s->part_slot;
        if (s->fading) { pit->h = (const float2*)s->d_fade_from; pit->h_to = (const float2*)s->d_fade_to; pit->fade_pos = s->fade_pos; pit->fade_len = s->fade_len; }
        else pit->h = (const float2*)s->d_fade_to;
        if (++s->part_slot == s->part_K) s->part_slot = 0;
    } else {
        it->ring = s->d_ring;
        it->head = s->rev_head;
        if (!xfade) it->ir = s->d_ir_mono;
        else if (s->fading) { it->ir = s->d_fade_from; it->ir_to = s->d_fade_to; it->fade_pos = s->fade_pos; it->fade_len = s->fade_len; }
        else it->ir = s->d_fade_to;
    }
    s->rev_head += (unsigned)frame;
    if (s->fading && (s->fade_pos += frame) >= s->fade_len) s->fading = false;   // complete: h_from := h_to, one convolution again
    return FS_OK;
}

// The pieces the two callbacks (reverb_rows, soundfield_rows) are built from.
// The rows by ascending Source*: the one locking order of every thread (fs_capi_publish.cpp).  A source that appears twice is
// refused, still before the first state change or enqueue.
int lock_order(fs_context* ctx, Source* const* srcs, int32_t count, std::vector<int32_t>* order) {
    order->resize((size_t)count);
    for (int32_t i = 0; i < count; ++i) (*order)[(size_t)i] = i;
    std::sort(order->begin(), order->end(), [&](int32_t a, int32_t b) { return srcs[a] < srcs[b]; });
    for (int32_t k = 1; k < count; ++k)
        if (srcs[(*order)[(size_t)k]] == srcs[(*order)[(size_t)k - 1]])
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a source appears twice in the batch");
    return FS_OK;
}
// The locks of all convolved sources (apply_reverb: null = every row), taken in that order.  They are held while the work is
// enqueued (a reconstruct that found one free would not wait for a read this call has yet to record), not longer.
std::vector<std::unique_lock<std::mutex>> lock_rows(Source* const* srcs, const std::vector<int32_t>& order, const int32_t* apply_reverb) {
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(order.size());
    for (int32_t i : order)
        if (!apply_reverb || apply_reverb[i]) locks.emplace_back(srcs[i]->ir_mu);
    return locks;
}
// One row kind's three lists in a staging block, [3][count] ints at `off` bytes on both sides: the rows with one product (or
// convolution), those with two, and those that take a newer IR in this callback.
struct RowLists {
    int* h; const int* d;
    int count, n_plain = 0, n_fade = 0, n_take = 0;
    RowLists(const CallbackStage& st, size_t off, int count_) : h((int*)(st.h + off)), d((const int*)(st.d + off)), count(count_) {}
    void add(int i, bool takes, bool fading) {
        if (takes) h[2 * count + n_take++] = i;
        if (fading) h[count + n_fade++] = i;
        else h[n_plain++] = i;
    }
    ReverbLists dev() const { return {d, n_plain, d + count, n_fade}; }
};
// launch(take, n_take) enqueues the take of the list's rows (when it has any); then every taken row's ev_rev is recorded behind it
template <class Launch>
int take_rows(fs_context* ctx, Source* const* srcs, const RowLists& l, hipStream_t rs, Launch launch) {
    if (!l.n_take) return FS_OK;
    launch(l.d + 2 * l.count, l.n_take);
    FS_HIP(ctx, hipGetLastError());
    for (int k = 0; k < l.n_take; ++k) FS_HIP(ctx, hipEventRecord(srcs[l.h[2 * l.count + k]]->ev_rev, rs));
    return FS_OK;
}

// The callback of `count` validated sources of one frame size (audio thread): one copy up, the launches, one copy back.
int reverb_rows(fs_context* ctx, Source* const* srcs, int32_t count, const float* in, float* out, const int32_t* apply_reverb,
                uint32_t flags, float* mix) {
    std::vector<int32_t> order;
    { const int rc = lock_order(ctx, srcs, count, &order); if (rc) return rc; }
    const int frame = srcs[0]->rev_frame;
    const size_t row = 2 * (size_t)frame;   // floats
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    bool ears = false;
    for (int32_t i = 0; i < count; ++i) ears = ears || (srcs[i]->rev_ears && (!apply_reverb || apply_reverb[i]));
    const size_t lists = sizeof(int) * 3 * (size_t)count;
    const CallbackLayout l = callback_layout(count, frame, 2 * (size_t)frame, {sizeof(ReverbItem) * (size_t)count, sizeof(ReverbPartItem) * (size_t)count, 2 * lists,
                                                            ears ? lists : 0},
                                             {sizeof(float) * row * (size_t)count});
    { const int rc = ctx->rev_stage.fit(ctx, l.host_bytes, l.dev_bytes); if (rc) return rc; }
    char* hs = ctx->rev_stage.h; char* ds = ctx->rev_stage.d;
    ReverbItem* items = (ReverbItem*)(hs + l.up[kRevItems]);
    ReverbPartItem* pitems = (ReverbPartItem*)(hs + l.up[kRevPartItems]);
    RowLists direct(ctx->rev_stage, l.up[kRevLists], count), part(ctx->rev_stage, l.up[kRevLists] + lists, count);
    RowLists ear(ctx->rev_stage, l.up[kRevEarLists], count);   // (rows only with ears)
    int n_bypass = 0;
    const Source* part_src = nullptr;
    float* h_in = (float*)(hs + l.in);
    for (int32_t i = 0; i < count; ++i)   // (a bypassed row goes up only for the mix)
        if (mix || !apply_reverb || apply_reverb[i])
            std::memcpy(h_in + (size_t)i * row, in + (size_t)i * row, sizeof(float) * row);
    {
        const auto locks = lock_rows(srcs, order, apply_reverb);
        for (int32_t i = 0; i < count; ++i) {   // the steps in list order
            std::memset(&items[i], 0, sizeof(ReverbItem));
            std::memset(&pitems[i], 0, sizeof(ReverbPartItem));
            if (apply_reverb && !apply_reverb[i]) { ++n_bypass; continue; }   // the bypass touches no state
            Source* s = srcs[i];
            const bool p = partitioned(s);
            items[i].apply = 1;
            items[i].engine = s->rev_engine;   // (of a partitioned row's ReverbItem the kernels read these two only)
            bool takes = false;
            const int rc = reverb_step(ctx, s, rs, frame, p ? nullptr : &items[i], p ? &pitems[i] : nullptr, &takes);
            if (rc) return rc;
            if (p) part_src = s;
            if (!p) direct.add(i, takes, items[i].ir_to != nullptr);
            else (s->rev_ears ? ear : part).add(i, takes, pitems[i].h_to != nullptr);
        }
        FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
        ReverbBatch b{};
        b.items = (const ReverbItem*)(ds + l.up[kRevItems]);
        { const int rc = take_rows(ctx, srcs, direct, rs, [&](const int* take, int n) { launch_reverb_batch_fade_start(b.items, take, n, ctx->num_samples, rs); }); if (rc) return rc; }
        if (part_src) {   // (one frame size and one context: N and K are those of every partitioned row)
            b.pitems = (const ReverbPartItem*)(ds + l.up[kRevPartItems]);
            b.part = ReverbShape{ctx->d_rev_tw[part_src->part_n], part_src->part_n, part_src->part_K, frame, ctx->num_samples};
            b.part_rows = part.dev();
            { const int rc = take_rows(ctx, srcs, part, rs, [&](const int* take, int n) { launch_reverb_part_take(b.pitems, take, n, b.part, rs); }); if (rc) return rc; }
            if (ears) {
                b.ear_rows = ear.dev();
                const ReverbEars e{ctx->d_ear_carrier, ctx->cfg.num_bands, carrier_stride(ctx->num_samples)};
                const int rc = take_rows(ctx, srcs, ear, rs, [&](const int* take, int n) { launch_reverb_ears_take(b.pitems, take, n, b.part, e, rs); });
                if (rc) return rc;
            }
        }
        b.n_direct = direct.n_plain + direct.n_fade + n_bypass;
        b.plain = direct.dev().plain; b.n_plain = direct.n_plain;
        b.fade = direct.dev().fade; b.n_fade = direct.n_fade;
        b.count = count; b.frame = frame; b.ir_size = ctx->num_samples;
        b.literal_tail = (flags & FS_REVERB_LITERAL_TAIL) ? 1 : 0;
        b.in = (const float*)(ds + l.in);
        b.cur = (float*)(ds + l.scratch[0]);
        b.out = (float*)(ds + l.d_out);
        b.mix = mix ? (float*)(ds + l.d_mix) : nullptr;
        launch_reverb_batch(b, rs);
        FS_HIP(ctx, hipGetLastError());
        for (int k = 0; k < direct.n_plain; ++k) {   // without a crossfade the convolution itself reads d_ir_mono
            Source* s = srcs[direct.h[k]];
            if (s->fade_len == 0) FS_HIP(ctx, hipEventRecord(s->ev_rev, rs));
        }
    }
    { const int rc = callback_finish(ctx, ctx->rev_stage, l, out != nullptr, mix); if (rc) return rc; }
    if (out) {   // row by row: a bypassed row comes from in, and the call may be in place
        const float* h_out = (const float*)(hs + l.h_out);
        for (int32_t i = 0; i < count; ++i) {   // bApplyReverb == false: RVB.cpp:128-132
            const float* from = (apply_reverb && !apply_reverb[i]) ? in + (size_t)i * row : h_out + (size_t)i * row;
            if (from != out + (size_t)i * row) std::memcpy(out + (size_t)i * row, from, sizeof(float) * row);   // (in place: in == out)
        }
    }
    return FS_OK;
}

// what the soundfield kernels read of the set in force
ReverbSoundfield soundfield_set(const fs_context* ctx) {
    ReverbSoundfield e{};
    e.c = ctx->d_sf_carrier;
    e.B = ctx->cfg.num_bands;
    e.ld = carrier_stride(ctx->num_samples);
    e.C = (ctx->sf_order + 1) * (ctx->sf_order + 1);
    for (int l = 0; l < 4; ++l) e.w[l] = 1.0f / sqrtf((float)(2 * l + 1));   // (w[0] = 1.0f exactly)
    return e;
}

// sf_stage's own blocks
enum { kSfItems, kSfLists };

// reverb_rows for `count` validated soundfield sources of one frame size (fs_reverb_soundfield_process_batch, audio thread): the
// same steps, locks and events, with rows of C frame floats coming back and no bypass, literal tail or clamp.
int soundfield_rows(fs_context* ctx, Source* const* srcs, int32_t count, const float* in, float* out, float* mix) {
    std::vector<int32_t> order;
    { const int rc = lock_order(ctx, srcs, count, &order); if (rc) return rc; }
    const int frame = srcs[0]->rev_frame;
    const ReverbSoundfield e = soundfield_set(ctx);
    const size_t in_row = 2 * (size_t)frame, row = (size_t)e.C * (size_t)frame;   // floats
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    const CallbackLayout l = callback_layout(count, frame, row, {sizeof(ReverbPartItem) * (size_t)count, sizeof(int) * 3 * (size_t)count}, {});
    { const int rc = ctx->sf_stage.fit(ctx, l.host_bytes, l.dev_bytes); if (rc) return rc; }
    char* hs = ctx->sf_stage.h; char* ds = ctx->sf_stage.d;
    ReverbPartItem* pitems = (ReverbPartItem*)(hs + l.up[kSfItems]);
    RowLists rows(ctx->sf_stage, l.up[kSfLists], count);
    std::memcpy(hs + l.in, in, sizeof(float) * in_row * (size_t)count);
    {
        const auto locks = lock_rows(srcs, order, nullptr);
        for (int32_t i = 0; i < count; ++i) {
            std::memset(&pitems[i], 0, sizeof(ReverbPartItem));
            bool takes = false;
            const int rc = reverb_step(ctx, srcs[i], rs, frame, nullptr, &pitems[i], &takes);
            if (rc) return rc;
            rows.add(i, takes, pitems[i].h_to != nullptr);
        }
        FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
        const ReverbPartItem* d_items = (const ReverbPartItem*)(ds + l.up[kSfItems]);
        const ReverbShape shape{ctx->d_rev_tw[srcs[0]->part_n], srcs[0]->part_n, srcs[0]->part_K, frame, ctx->num_samples};
        { const int rc = take_rows(ctx, srcs, rows, rs, [&](const int* take, int n) { launch_reverb_soundfield_take(d_items, take, n, shape, e, rs); }); if (rc) return rc; }
        launch_reverb_soundfield(d_items, shape, rows.dev(), e, count, (const float*)(ds + l.in), (float*)(ds + l.d_out),
                                 mix ? (float*)(ds + l.d_mix) : nullptr, rs);
        FS_HIP(ctx, hipGetLastError());
    }
    { const int rc = callback_finish(ctx, ctx->sf_stage, l, out != nullptr, mix); if (rc) return rc; }
    if (out) std::memcpy(out, hs + l.h_out, sizeof(float) * row * (size_t)count);
    return FS_OK;
}

// The per-row validation of the two batch entry points: soundfield says whose rows the call takes.  Everything is validated before
// the first state change or enqueue: a refused call changes nothing.
int batch_sources(fs_context* ctx, const fs_source* sources, int32_t count, bool soundfield, const int32_t* apply_reverb,
                  std::vector<Source*>* srcs) {
    srcs->resize((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        Source* s = (*srcs)[(size_t)i] = get_source(ctx, sources[i]);
        if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
        if (!s->d_ring) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init has not been called for this source");
        if (s->rev_sf != soundfield)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, soundfield ? "the source is not initialised with the soundfield (fs_reverb_set_soundfield, then fs_reverb_init)"
                                                                 : kSoundfieldSource);
        if (s->rev_frame != (*srcs)[0]->rev_frame) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "the sources of a batch share one frame size");
        const bool missing = soundfield ? !s->d_fade_to || (s->fade_len > 0 && !s->d_fade_from)
                                        : (!apply_reverb || apply_reverb[i]) && s->fade_len > 0 && (!s->d_fade_from || !s->d_fade_to);
        if (missing) return ctx->fail(FS_ERR_OUT_OF_MEMORY, kNoFadeBuffers);
    }
    return FS_OK;
}

// The two IR-copy entry points: launch(bands, d) writes the source's IRs, `floats` of them, to the device block d; they come back
// as dst[k] <- d [k * each .. (k + 1) * each)
template <class Launch>
int copy_irs(fs_context* ctx, fs_source h, int32_t n, const float* carriers, const char* what, const char* no_set, size_t floats,
             std::initializer_list<float*> dst, Launch launch) {
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (n != ctx->num_samples) return ctx->fail(FS_ERR_SIZE_MISMATCH, "n != num_samples");
    if (!carriers) return ctx->fail(FS_ERR_INVALID_ARGUMENT, std::string(what) + no_set);
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    FS_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));   // the reconstruct runs on the tail stream
    float* d = nullptr;
    FS_HIP(ctx, hipMalloc((void**)&d, sizeof(float) * floats));
    launch(s->d_ir_bands, d);
    hipError_t err = hipGetLastError();
    const size_t each = floats / dst.size();
    size_t k = 0;
    for (float* to : dst)
        if (err == hipSuccess) err = hipMemcpyAsync(to, d + each * k++, sizeof(float) * each, hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (err != hipSuccess) return ctx->hip_fail(err, what);
    return FS_OK;
}

}  // namespace

int CallbackStage::fit(fs_context* ctx, size_t host_bytes, size_t dev_bytes) {
    if (host_bytes <= host_cap && dev_bytes <= dev_cap) return FS_OK;
    // first call of this size (every call ends synchronised: nothing reads the old pair)
    const size_t hb = std::max(host_bytes, host_cap), db = std::max(dev_bytes, dev_cap);
    release();
    FS_HIP(ctx, hipHostMalloc((void**)&h, hb, hipHostMallocDefault));
    host_cap = hb;
    FS_HIP(ctx, hipMalloc((void**)&d, db));
    dev_cap = db;
    return FS_OK;
}

void CallbackStage::release() {
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    h = d = nullptr; host_cap = dev_cap = 0;
}

namespace fsi {

CallbackLayout callback_layout(int count, int frame, size_t out_row, std::initializer_list<size_t> up_blocks,
                               std::initializer_list<size_t> scratch_blocks) {
    auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
    CallbackLayout l;
    l.in_rows = sizeof(float) * 2 * (size_t)frame * (size_t)count;
    l.row = sizeof(float) * out_row;
    l.rows = l.row * (size_t)count;
    int k = 0;
    for (size_t bytes : up_blocks) { l.up[k++] = l.in; l.in += align(bytes); }
    l.up_bytes = l.in + l.in_rows;
    l.h_out = align(l.up_bytes);
    l.h_mix = l.h_out + l.rows;   // (adjacent to out: rows is a multiple of 4 bytes)
    l.host_bytes = l.h_mix + l.row;
    l.d_out = align(l.up_bytes);
    k = 0;
    for (size_t bytes : scratch_blocks) { l.scratch[k++] = l.d_out; l.d_out += align(bytes); }
    l.d_mix = l.d_out + l.rows;
    l.dev_bytes = l.d_mix + l.row;
    return l;
}

int callback_finish(fs_context* ctx, const CallbackStage& st, const CallbackLayout& l, bool want_out, float* mix) {
    hipStream_t rs = ctx->rev_stream;
    if (want_out)   // out | mix are adjacent on both sides: one copy back
        FS_HIP(ctx, hipMemcpyAsync(st.h + l.h_out, st.d + l.d_out, l.rows + (mix ? l.row : 0), hipMemcpyDeviceToHost, rs));
    else
        FS_HIP(ctx, hipMemcpyAsync(st.h + l.h_mix, st.d + l.d_mix, l.row, hipMemcpyDeviceToHost, rs));
    FS_HIP(ctx, hipStreamSynchronize(rs));
    if (mix) std::memcpy(mix, st.h + l.h_mix, l.row);
    return FS_OK;
}

}  // namespace fsi

extern "C" {

int fs_reverb_init(fs_context* ctx, fs_source h, int32_t frame_size) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    const bool part = s->rev_engine_next == FS_REVERB_ENGINE_PARTITIONED;
    if (part) {
        if (frame_size < 16 || frame_size > 2048 || ctx->num_samples > 1048576)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "partitioned reverb: frame size outside 16 .. 2048 / IR longer than 1 048 576 samples");
    } else if (frame_size < 1 || frame_size > 16384 || ctx->num_samples - 1 > kReverbRing)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad reverb frame size / IR longer than the history ring");
    if (s->rev_ears_next && !part)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init: ears are on (fs_reverb_set_ears) but the source's engine is not FS_REVERB_ENGINE_PARTITIONED");
    if (s->rev_ears_next && !ctx->d_ear_carrier)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init: ears are on (fs_reverb_set_ears) but no ear set is installed (fs_reverb_ears_set)");
    if (s->rev_sf_next && !part)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init: the soundfield is on (fs_reverb_set_soundfield) but the source's engine is not FS_REVERB_ENGINE_PARTITIONED");
    if (s->rev_sf_next && !ctx->d_sf_carrier)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init: the soundfield is on (fs_reverb_set_soundfield) but no soundfield set is installed (fs_reverb_soundfield_set)");
    if (s->rev_sf_next && s->rev_ears_next)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init: the soundfield (fs_reverb_set_soundfield) and ears (fs_reverb_set_ears) are both on: a source has one of them");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    // Reconstructs on the compute stream record an event for the callbacks only for a source that has a reverb: the ones
    // already in flight finish before this source gets one.
    FS_FLUSH(ctx);
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->rev_stream));
    if (s->d_ring) (void)hipFree(s->d_ring);
    if (s->d_fade_from) (void)hipFree(s->d_fade_from);
    if (s->d_fade_to) (void)hipFree(s->d_fade_to);
    s->d_ring = s->d_fade_from = s->d_fade_to = nullptr;
    s->rev_engine = s->rev_engine_next;
    s->rev_ears = s->rev_ears_next;
    s->rev_sf = s->rev_sf_next;
    s->part_sets = s->rev_sf ? ((ctx->sf_order + 1) * (ctx->sf_order + 1) + 1) / 2 : s->rev_ears ? 2 : 1;
    if (part) {   // N = the smallest power of two >= 2 F, K = ceil(num_samples / F)
        s->part_n = 5;
        while ((1 << s->part_n) < 2 * frame_size) ++s->part_n;
        s->part_K = (ctx->num_samples + frame_size - 1) / frame_size;
        const int rc = part_twiddles(ctx, s->part_n);
        if (rc) return rc;
    }
    const size_t ring_bytes = reverb_state_bytes(s);
    FS_HIP(ctx, hipMalloc((void**)&s->d_ring, ring_bytes));
    FS_HIP(ctx, hipMemsetAsync(s->d_ring, 0, ring_bytes, ctx->rev_stream));   // SetNumZeroed
    s->rev_head = 0;
    s->part_slot = 0;
    s->rev_frame = frame_size;
    s->fading = s->fade_primed = false;   // (the first callback takes the IR unfaded)
    if (s->fade_len > 0 || part) return alloc_fade(ctx, s, s->fade_len > 0);
    return FS_OK;
}

int fs_reverb_set_engine(fs_context* ctx, fs_source h, int32_t engine) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (engine != FS_REVERB_ENGINE_DIRECT && engine != FS_REVERB_ENGINE_PARTITIONED)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "unknown reverb engine (FS_REVERB_ENGINE_DIRECT, FS_REVERB_ENGINE_PARTITIONED)");
    s->rev_engine_next = engine;   // (the next fs_reverb_init's)
    return FS_OK;
}

void fs_reverb_ears_default(fs_reverb_ears_desc* d) {
    if (!d) return;
    d->struct_size = (uint32_t)sizeof(fs_reverb_ears_desc);
    d->radius_cm = FS_HRTF_DEFAULT_RADIUS_CM;
    d->sound_speed_cm_s = FS_HRTF_DEFAULT_SOUND_SPEED_CM_S;
}

int fs_reverb_ears_set(fs_context* ctx, const fs_reverb_ears_desc* desc) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (!desc) {   // clear
        for (const Source* s : ctx->sources)
            if (s && s->alive && s->d_ring && s->rev_ears)
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_ears_set: the set cannot be cleared while a source is initialised with ears (fs_reverb_init it without them first)");
        if (!ctx->d_ear_carrier) return FS_OK;
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        return fsi::install_ear_carriers(ctx, nullptr, 0.0f, 0.0f);
    }
    if (desc->struct_size != sizeof(fs_reverb_ears_desc)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_ears_desc.struct_size mismatch");
    if (!std::isfinite(desc->radius_cm) || desc->radius_cm < 0.0f)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_ears_set: radius_cm must be finite and >= 0");
    if (!std::isfinite(desc->sound_speed_cm_s) || !(desc->sound_speed_cm_s > 0.0f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_ears_set: sound_speed_cm_s must be finite and > 0");
    { const int rc = fsi::check_band_edges(ctx, nullptr, "fs_reverb_ears_set"); if (rc) return rc; }
    { const int rc = fs_synchronize(ctx); if (rc) return rc; }   // (the build runs on the compute stream, behind everything in flight)
    float* set = nullptr;
    const int rc = fsi::build_ear_carriers(ctx, desc->radius_cm, desc->sound_speed_cm_s, "fs_reverb_ears_set", &set);
    if (rc) return rc;
    return fsi::install_ear_carriers(ctx, set, desc->radius_cm, desc->sound_speed_cm_s);
}

int fs_reverb_ears_info(fs_context* ctx, float* radius_cm, float* sound_speed_cm_s, int32_t* installed) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (radius_cm) *radius_cm = ctx->ear_radius_cm;
    if (sound_speed_cm_s) *sound_speed_cm_s = ctx->ear_speed_cm_s;
    if (installed) *installed = ctx->d_ear_carrier ? 1 : 0;
    return FS_OK;
}

int fs_reverb_set_ears(fs_context* ctx, fs_source h, int32_t on) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    s->rev_ears_next = on != 0;   // (the next fs_reverb_init's)
    return FS_OK;
}

int fs_reverb_copy_ear_impulse_responses(fs_context* ctx, fs_source h, float* left, float* right, int32_t n) {
    if (!ctx || !left || !right) return FS_ERR_INVALID_ARGUMENT;
    const ReverbEars e{ctx->d_ear_carrier, ctx->cfg.num_bands, carrier_stride(ctx->num_samples)};
    return copy_irs(ctx, h, n, e.c, "fs_reverb_copy_ear_impulse_responses", ": no ear set is installed (fs_reverb_ears_set)", 2 * (size_t)n,
                    {left, right}, [&](const float* bands, float* d) { launch_reverb_ears_ir(bands, e, n, d, d + n, ctx->stream); });
}

int fs_reverb_soundfield_set(fs_context* ctx, int32_t order) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (order < -1 || order > FS_MAX_AMBISONIC_ORDER)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_soundfield_set: order outside 0 .. FS_MAX_AMBISONIC_ORDER (-1: clear)");
    if (order == ctx->sf_order) return FS_OK;   // (the order installed, or nothing to clear: nothing changes)
    for (const Source* s : ctx->sources)
        if (s && s->alive && s->d_ring && s->rev_sf)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_soundfield_set: the set cannot be cleared or change its order while a source is initialised with the soundfield (fs_reverb_init it without first)");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (order < 0) return fsi::install_soundfield_carriers(ctx, nullptr, -1);
    { const int rc = fsi::check_band_edges(ctx, nullptr, "fs_reverb_soundfield_set"); if (rc) return rc; }
    { const int rc = fs_synchronize(ctx); if (rc) return rc; }   // (the build runs on the compute stream, behind everything in flight)
    float* set = nullptr;
    const int rc = fsi::build_soundfield_carriers(ctx, order, "fs_reverb_soundfield_set", &set);
    if (rc) return rc;
    return fsi::install_soundfield_carriers(ctx, set, order);
}

int fs_reverb_soundfield_info(fs_context* ctx, int32_t* order, int32_t* installed) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (order) *order = ctx->sf_order;
    if (installed) *installed = ctx->d_sf_carrier ? 1 : 0;
    return FS_OK;
}

int fs_reverb_set_soundfield(fs_context* ctx, fs_source h, int32_t on) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    s->rev_sf_next = on != 0;   // (the next fs_reverb_init's)
    return FS_OK;
}

int fs_reverb_copy_soundfield_impulse_responses(fs_context* ctx, fs_source h, float* out, int32_t n) {
    if (!ctx || !out) return FS_ERR_INVALID_ARGUMENT;
    const ReverbSoundfield e = soundfield_set(ctx);
    return copy_irs(ctx, h, n, e.c, "fs_reverb_copy_soundfield_impulse_responses", ": no soundfield set is installed (fs_reverb_soundfield_set)",
                    (size_t)e.C * (size_t)n, {out}, [&](const float* bands, float* d) { launch_reverb_soundfield_ir(bands, e, n, d, ctx->stream); });
}

int fs_reverb_soundfield_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in, float* out,
                                       uint32_t flags, float* mix) {
    if (!ctx || !sources || !in || (!out && !mix)) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (flags != 0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_soundfield_process_batch: flags must be 0");
    if (count < 1 || count > FS_MAX_REVERB_BATCH)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REVERB_BATCH)");
    std::vector<Source*> srcs;
    { const int rc = batch_sources(ctx, sources, count, true, nullptr, &srcs); if (rc) return rc; }
    return soundfield_rows(ctx, srcs.data(), count, in, out, mix);
}

int fs_reverb_set_crossfade(fs_context* ctx, fs_source h, int32_t samples) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (samples < 0 || (int64_t)samples > 4 * (int64_t)ctx->cfg.sample_rate)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "crossfade length out of range (0 = off, 1 .. 4 * sample_rate)");
    if (samples > 0 && s->d_ring) {
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        const int rc = alloc_fade(ctx, s, true);
        if (rc) return rc;
    }
    if (s->fade_len == 0) s->fade_primed = false;   // enabling: nothing to fade from
    s->fading = false;                              // a running fade ends at its target IR
    s->fade_len = samples;
    return FS_OK;
}

int fs_reverb_process(fs_context* ctx, fs_source h, const float* in, float* out, int32_t apply_reverb, uint32_t flags) {
    if (!ctx || !in || !out) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (!s->d_ring) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init has not been called for this source");
    if (s->rev_sf) return ctx->fail(FS_ERR_INVALID_ARGUMENT, kSoundfieldSource);
    if (!apply_reverb) {   // bApplyReverb == false: RVB.cpp:128-132 (neither the device nor any state; in == out is allowed)
        if (out != in) std::memmove(out, in, sizeof(float) * 2 * (size_t)s->rev_frame);
        return FS_OK;
    }
    if (s->fade_len > 0 && (!s->d_fade_from || !s->d_fade_to))   // (fs_reverb_init could not allocate them)
        return ctx->fail(FS_ERR_OUT_OF_MEMORY, kNoFadeBuffers);
    return reverb_rows(ctx, &s, 1, in, out, nullptr, flags, nullptr);
}

int fs_reverb_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in, float* out,
                            const int32_t* apply_reverb, uint32_t flags, float* mix) {
    if (!ctx || !sources || !in || (!out && !mix)) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (count < 1 || count > FS_MAX_REVERB_BATCH)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REVERB_BATCH)");
    std::vector<Source*> srcs;
    { const int rc = batch_sources(ctx, sources, count, false, apply_reverb, &srcs); if (rc) return rc; }
    return reverb_rows(ctx, srcs.data(), count, in, out, apply_reverb, flags, mix);
}

int fs_reverb_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (s->d_ring && ctx->device_ok) {
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        FS_HIP(ctx, hipMemsetAsync(s->d_ring, 0, reverb_state_bytes(s), ctx->rev_stream));   // (partitioned: the window history and the spectrum ring)
        s->rev_head = 0;
        s->part_slot = 0;
        s->fading = false;   // a running crossfade ends at its target IR
    }
    return FS_OK;
}

}  // extern "C"
