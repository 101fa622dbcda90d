// fs_capi_reflect_render.cpp — the early reflections on the audio thread: the per-source set-up (fs_reflection_render_init /
// _release) and the callback of all sources (fs_reflection_render_process_batch: everything validated, the voices matched to the
// slots on the host's copy of the slot table, one copy up, the launches of fs_reflect_render.hip, one copy back, one wait).  The
// band kernels and their per-context cache are the direct renderer's (fs_capi_direct_render.cpp).  The reference has no slot for it.
#include "fs_context.hpp"

static_assert(sizeof(fs_reflection_voice) == 48, "fs_reflection_voice: the key, the delay, the bands, two channels");
static_assert(sizeof(fs_reflection_render_row) == 16, "fs_reflection_render_row: four counts");

namespace {

// The staging of one callback (fs_context::h_rr_stage / d_rr_stage), every block 256-byte aligned
struct RrStageLayout {
    size_t items, voices, in, up_bytes;            // host and device, the same offsets: what goes up in one copy
    size_t h_out, h_mix, host_bytes;               // host: what comes back
    size_t d_n0, d_plans, d_out, d_mix, dev_bytes; // device: out | mix adjacent, one copy back
};
size_t rr_align(size_t b) { return (b + 255) & ~(size_t)255; }
RrStageLayout rr_stage_layout(int count, int stride, int frame) {
    const size_t rows = sizeof(float) * 2 * (size_t)frame * (size_t)count, row = sizeof(float) * 2 * (size_t)frame;
    RrStageLayout l;
    l.items = 0;
    l.voices = rr_align(sizeof(ReflectRenderItem) * (size_t)count);
    l.in = l.voices + rr_align(sizeof(fs_reflection_voice) * (size_t)count * (size_t)stride);
    l.up_bytes = l.in + rows;
    l.h_out = rr_align(l.up_bytes);
    l.h_mix = l.h_out + rows;   // (adjacent to out)
    l.host_bytes = l.h_mix + row;
    l.d_n0 = rr_align(l.up_bytes);
    l.d_plans = l.d_n0 + rr_align(sizeof(unsigned) * (size_t)count);
    l.d_out = l.d_plans + rr_align(sizeof(ReflectRenderPlan) * (size_t)count * FS_MAX_REFLECTION_VOICES);
    l.d_mix = l.d_out + rows;
    l.dev_bytes = l.d_mix + row;
    return l;
}

size_t rr_state_bytes(const Source* s) { return kReflectRenderHeader + sizeof(float) * 2 * (size_t)s->rr_ring; }

void rr_free_slots(Source* s) {
    for (int j = 0; j < FS_MAX_REFLECTION_VOICES; ++j) { s->rr_held[j] = false; s->rr_key[j] = 0; }
}

// what one row's matching decides: the slots' ops, the table afterwards, the counts
struct RrMatch {
    int8_t op[FS_MAX_REFLECTION_VOICES];
    bool held[FS_MAX_REFLECTION_VOICES];
    uint32_t key[FS_MAX_REFLECTION_VOICES];
    fs_reflection_render_row row;
};

// Rule 1 of the header: held slots continue or end by their key; the other entries start, in list order, on the lowest slot that
// was free when the callback began; what finds none is dropped.  (n entries with distinct keys: checked by the caller.)
RrMatch rr_match(const Source* s, const fs_reflection_voice* v, int n) {
    RrMatch m{};
    const int V = s->rr_voices;
    bool taken[FS_MAX_REFLECTION_VOICES] = {};   // entries a held slot continues with
    for (int j = 0; j < FS_MAX_REFLECTION_VOICES; ++j) m.op[j] = (int8_t)kReflectIdle;
    for (int j = 0; j < V; ++j) {
        if (!s->rr_held[j]) continue;
        int e = 0;
        while (e < n && v[e].key != s->rr_key[j]) ++e;
        if (e < n) {
            m.op[j] = (int8_t)(kReflectContinue + e);
            m.held[j] = true; m.key[j] = s->rr_key[j];
            taken[e] = true;
        } else {
            m.op[j] = (int8_t)kReflectEnd;
            m.row.ended++;
        }
        m.row.sounding++;
    }
    int next = 0;   // the lowest slot not looked at yet
    for (int e = 0; e < n; ++e) {
        if (taken[e]) continue;
        while (next < V && s->rr_held[next]) ++next;   // (an ending slot is held during this callback)
        if (next == V) { m.row.dropped++; continue; }
        m.op[next] = (int8_t)(kReflectStart + e);
        m.held[next] = true; m.key[next] = v[e].key;
        m.row.started++; m.row.sounding++;
        ++next;
    }
    return m;
}

}  // namespace

extern "C" {

int fs_reflection_render_init(fs_context* ctx, fs_source h, int32_t frame_size, int32_t taps, int32_t voices, float max_delay_seconds) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (frame_size < 16 || frame_size > 16384 || !direct_render_taps_ok(taps) || voices < 1 || voices > FS_MAX_REFLECTION_VOICES ||
        !std::isfinite(max_delay_seconds) || !(max_delay_seconds >= 0.0f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reflection_render_init: frame size outside 16 .. 16384, taps even or outside 1 .. 2047, voices outside 1 .. 32, or a bad max delay");
    const double d_max = std::ceil((double)max_delay_seconds * (double)ctx->cfg.sample_rate);
    const double need = d_max + (double)taps + 1.0 + (double)frame_size;
    if (need > 1048576.0)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reflection_render_init: max delay + taps + 1 + frame size exceed 1 048 576 samples");
    unsigned ring = 1;
    while ((double)ring < need) ring <<= 1;
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const float* table = nullptr;
    const int rc = direct_render_table_for(ctx, taps, &table);
    if (rc) return rc;
    FS_HIP(ctx, hipStreamSynchronize(ctx->rev_stream));
    if (s->d_rr) (void)hipFree(s->d_rr);
    s->d_rr = nullptr;
    s->rr_frame = frame_size;
    s->rr_taps = taps;
    s->rr_voices = voices;
    s->rr_max_delay = (int)d_max;
    s->rr_ring = ring;
    s->rr_table = table;
    rr_free_slots(s);
    FS_HIP(ctx, hipMalloc((void**)&s->d_rr, rr_state_bytes(s)));
    FS_HIP(ctx, hipMemsetAsync(s->d_rr, 0, rr_state_bytes(s), ctx->rev_stream));
    return FS_OK;
}

int fs_reflection_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (s->d_rr && ctx->device_ok) {   // history := 0, every slot free
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        FS_HIP(ctx, hipMemsetAsync(s->d_rr, 0, rr_state_bytes(s), ctx->rev_stream));
        rr_free_slots(s);
    }
    return FS_OK;
}

int fs_reflection_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                                       const fs_reflection_voice* voices, const int32_t* voice_counts, int32_t stride, float* out,
                                       float* mix, fs_reflection_render_row* rows) {
    if (!ctx || !sources || !in || !voices || !voice_counts || (!out && !mix)) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (count < 1 || count > FS_MAX_REFLECTION_RENDER_BATCH)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REFLECTION_RENDER_BATCH)");
    if (stride < 1 || stride > FS_MAX_REFLECTION_VOICES)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "stride out of range (1 .. FS_MAX_REFLECTION_VOICES)");
    // Everything is validated before the first state change or enqueue: a refused call changes nothing.
    const int B = ctx->cfg.num_bands;
    const float fs_f = (float)ctx->cfg.sample_rate;
    std::vector<Source*> srcs((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        Source* s = srcs[(size_t)i] = get_source(ctx, sources[i]);
        if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
        if (!s->d_rr) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reflection_render_init has not been called for this source");
        if (s->rr_frame != srcs[0]->rr_frame || s->rr_taps != srcs[0]->rr_taps)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "the sources of a batch share one frame size and one tap count");
        const int32_t n = voice_counts[i];
        if (n < 0 || n > stride) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice count outside 0 .. stride");
        const fs_reflection_voice* v = voices + (size_t)i * (size_t)stride;
        for (int32_t e = 0; e < n; ++e) {
            for (int32_t f = 0; f < e; ++f)
                if (v[f].key == v[e].key) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a key appears twice in one row");
            if (!std::isfinite(v[e].delay) || !(v[e].delay >= 0.0f) || v[e].delay * fs_f > (float)s->rr_max_delay)
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's delay is negative, not finite or beyond the source's max delay");
            for (int b = 0; b < B; ++b)
                if (!std::isfinite(v[e].band_gain[b]) || !(v[e].band_gain[b] >= 0.0f))
                    return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's band gain is negative or not finite");
            if (!std::isfinite(v[e].channel_gain[0]) || !std::isfinite(v[e].channel_gain[1]))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's channel gain is not finite");
        }
    }
    {
        std::vector<Source*> sorted(srcs);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a source appears twice in the batch");
    }
    const int frame = srcs[0]->rr_frame;
    const size_t row = 2 * (size_t)frame;   // floats
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    const RrStageLayout l = rr_stage_layout(count, stride, frame);
    if (l.host_bytes > ctx->rr_stage_host || l.dev_bytes > ctx->rr_stage_dev) {   // first call of this size (every call ends synchronised: nothing reads the old one)
        // (both grow to the largest seen: the two do not grow in step when count x stride and count x frame_size vary apart)
        const size_t hb = std::max(l.host_bytes, ctx->rr_stage_host), db = std::max(l.dev_bytes, ctx->rr_stage_dev);
        if (ctx->h_rr_stage) (void)hipHostFree(ctx->h_rr_stage);
        if (ctx->d_rr_stage) (void)hipFree(ctx->d_rr_stage);
        ctx->h_rr_stage = ctx->d_rr_stage = nullptr; ctx->rr_stage_host = ctx->rr_stage_dev = 0;
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_rr_stage, hb, hipHostMallocDefault));
        ctx->rr_stage_host = hb;
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_rr_stage, db));
        ctx->rr_stage_dev = db;
    }
    char* hs = ctx->h_rr_stage; char* ds = ctx->d_rr_stage;
    ReflectRenderItem* items = (ReflectRenderItem*)(hs + l.items);
    std::vector<RrMatch> matches((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = srcs[(size_t)i];
        RrMatch& m = matches[(size_t)i] = rr_match(s, voices + (size_t)i * (size_t)stride, voice_counts[i]);
        ReflectRenderItem& it = items[i];
        std::memset(&it, 0, sizeof(it));
        it.state = (ReflectRenderState*)s->d_rr;
        it.ring = (float*)(s->d_rr + kReflectRenderHeader);
        it.table = s->rr_table;
        it.mask = s->rr_ring - 1u;
        it.slots = s->rr_voices;
        std::memcpy(it.op, m.op, sizeof(it.op));
    }
    std::memcpy(hs + l.voices, voices, sizeof(fs_reflection_voice) * (size_t)count * (size_t)stride);
    std::memcpy(hs + l.in, in, sizeof(float) * row * (size_t)count);
    FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
    ReflectRenderBatch b{};
    b.items = (const ReflectRenderItem*)(ds + l.items);
    b.voices = (const fs_reflection_voice*)(ds + l.voices);
    b.plans = (ReflectRenderPlan*)(ds + l.d_plans);
    b.n0 = (unsigned*)(ds + l.d_n0);
    b.count = count; b.stride = stride; b.frame = frame; b.taps = srcs[0]->rr_taps; b.bands = B;
    b.fs = fs_f;
    b.in = (const float*)(ds + l.in);
    b.out = (float*)(ds + l.d_out);
    b.mix = mix ? (float*)(ds + l.d_mix) : nullptr;
    launch_reflect_render(b, rs);
    FS_HIP(ctx, hipGetLastError());
    for (int32_t i = 0; i < count; ++i) {   // the plan pass is on its way: the slot tables are what it leaves behind
        Source* s = srcs[(size_t)i];
        std::memcpy(s->rr_held, matches[(size_t)i].held, sizeof(s->rr_held));
        std::memcpy(s->rr_key, matches[(size_t)i].key, sizeof(s->rr_key));
    }
    if (out)   // out | mix are adjacent on both sides: one copy back
        FS_HIP(ctx, hipMemcpyAsync(hs + l.h_out, ds + l.d_out, sizeof(float) * row * ((size_t)count + (mix ? 1 : 0)), hipMemcpyDeviceToHost, rs));
    else
        FS_HIP(ctx, hipMemcpyAsync(hs + l.h_mix, ds + l.d_mix, sizeof(float) * row, hipMemcpyDeviceToHost, rs));
    FS_HIP(ctx, hipStreamSynchronize(rs));
    if (out) std::memcpy(out, hs + l.h_out, sizeof(float) * row * (size_t)count);
    if (mix) std::memcpy(mix, hs + l.h_mix, sizeof(float) * row);
    if (rows)
        for (int32_t i = 0; i < count; ++i) rows[i] = matches[(size_t)i].row;
    return FS_OK;
}

}  // extern "C"
