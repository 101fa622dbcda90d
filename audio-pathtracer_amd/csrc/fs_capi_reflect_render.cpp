// fs_capi_reflect_render.cpp — the early reflections on the audio thread: the per-source set-up (fs_reflection_render_init /
// _release) and the callback of all sources (fs_reflection_render_process_batch: everything validated, the voices matched to the
// slots on the host's copy of the slot table, one copy up, the launches of fs_reflect_render.hip, one copy back, one wait).  The
// band kernels and their per-context cache are the direct renderer's (fs_capi_direct_render.cpp).  The reference has no slot for it.
#include "fs_context.hpp"

static_assert(sizeof(fs_reflection_voice) == 48, "fs_reflection_voice: the key, the delay, the bands, two channels");
static_assert(sizeof(fs_reflection_render_row) == 16, "fs_reflection_render_row: four counts");

namespace {

void rr_free_slots(Source* s) {
    for (int j = 0; j < FS_MAX_REFLECTION_VOICES; ++j) { s->rr_held[j] = false; s->rr_key[j] = 0; }
}

}  // namespace

namespace fsi {

// Rule 1 of the header: held slots continue or end by their key; the other entries start, in list order, on the lowest slot that
// was free when the callback began; what finds none is dropped.  (n entries with distinct keys: checked by the caller.)
VoiceMatch voice_match(const bool* held, const uint32_t* key, int V, const void* voices, size_t voice_bytes, int n) {
    VoiceMatch m{};
    auto key_of = [&](int e) { uint32_t k; std::memcpy(&k, (const char*)voices + (size_t)e * voice_bytes, sizeof(k)); return k; };
    bool taken[FS_MAX_REFLECTION_VOICES] = {};   // entries a held slot continues with
    for (int j = 0; j < FS_MAX_REFLECTION_VOICES; ++j) m.op[j] = (int8_t)kReflectIdle;
    for (int j = 0; j < V; ++j) {
        if (!held[j]) continue;
        int e = 0;
        while (e < n && key_of(e) != key[j]) ++e;
        if (e < n) {
            m.op[j] = (int8_t)(kReflectContinue + e);
            m.held[j] = true; m.key[j] = key[j];
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
        while (next < V && held[next]) ++next;   // (an ending slot is held during this callback)
        if (next == V) { m.row.dropped++; continue; }
        m.op[next] = (int8_t)(kReflectStart + e);
        m.held[next] = true; m.key[next] = key_of(e);
        m.row.started++; m.row.sounding++;
        ++next;
    }
    return m;
}

}  // namespace fsi

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
    const int rc = render_setup(ctx, s->rr, kReflectRenderHeader, frame_size, taps, d_max, need);
    if (rc) return rc;   // (without a set-up, or with the old one untouched)
    s->rr_voices = voices;
    rr_free_slots(s);
    return FS_OK;
}

int fs_reflection_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    const int rc = render_clear(ctx, s->rr, kReflectRenderHeader);   // history := 0 ...
    if (rc == FS_OK) rr_free_slots(s);                                // ... every slot free
    return rc;
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
        int rc;
        Source* s = srcs[(size_t)i] = render_row(ctx, sources[i], &Source::rr, "fs_reflection_render_init has not been called for this source", i ? srcs[0] : nullptr, &rc);
        if (rc) return rc;
        const int32_t n = voice_counts[i];
        if (n < 0 || n > stride) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice count outside 0 .. stride");
        const fs_reflection_voice* v = voices + (size_t)i * (size_t)stride;
        for (int32_t e = 0; e < n; ++e) {
            for (int32_t f = 0; f < e; ++f)
                if (v[f].key == v[e].key) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a key appears twice in one row");
            rc = render_aim_check(ctx, "voice", v[e].delay, v[e].band_gain, s->rr);
            if (rc) return rc;
            if (!std::isfinite(v[e].channel_gain[0]) || !std::isfinite(v[e].channel_gain[1]))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's channel gain is not finite");
        }
    }
    { const int rc = render_no_duplicates(ctx, srcs); if (rc) return rc; }
    const int frame = srcs[0]->rr.frame;
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    enum { kItems, kVoices, kN0 = 0, kPlans };   // CallbackLayout::up and ::scratch
    const CallbackLayout l = callback_layout(count, frame, {sizeof(ReflectRenderItem) * (size_t)count, sizeof(fs_reflection_voice) * (size_t)count * (size_t)stride},
                                             {sizeof(unsigned) * (size_t)count, sizeof(ReflectRenderPlan) * (size_t)count * FS_MAX_REFLECTION_VOICES});
    { const int rc = ctx->rr_stage.fit(ctx, l.host_bytes, l.dev_bytes); if (rc) return rc; }
    char* hs = ctx->rr_stage.h; char* ds = ctx->rr_stage.d;
    ReflectRenderItem* items = (ReflectRenderItem*)(hs + l.up[kItems]);
    std::vector<VoiceMatch> matches((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = srcs[(size_t)i];
        VoiceMatch& m = matches[(size_t)i] = voice_match(s->rr_held, s->rr_key, s->rr_voices, voices + (size_t)i * (size_t)stride, sizeof(fs_reflection_voice), voice_counts[i]);
        ReflectRenderItem& it = items[i];
        std::memset(&it, 0, sizeof(it));
        it.state = (ReflectRenderState*)s->rr.d;
        it.ring = (float*)(s->rr.d + kReflectRenderHeader);
        it.table = s->rr.table;
        it.mask = s->rr.ring - 1u;
        it.slots = s->rr_voices;
        std::memcpy(it.op, m.op, sizeof(it.op));
    }
    std::memcpy(hs + l.up[kVoices], voices, sizeof(fs_reflection_voice) * (size_t)count * (size_t)stride);
    std::memcpy(hs + l.in, in, l.rows);
    FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
    ReflectRenderBatch b{};
    b.items = (const ReflectRenderItem*)(ds + l.up[kItems]);
    b.voices = (const fs_reflection_voice*)(ds + l.up[kVoices]);
    b.plans = (ReflectRenderPlan*)(ds + l.scratch[kPlans]);
    b.n0 = (unsigned*)(ds + l.scratch[kN0]);
    b.count = count; b.stride = stride; b.frame = frame; b.taps = srcs[0]->rr.taps; b.bands = B;
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
    { const int rc = callback_finish(ctx, ctx->rr_stage, l, out != nullptr, mix); if (rc) return rc; }
    if (out) std::memcpy(out, hs + l.h_out, l.rows);
    if (rows)
        for (int32_t i = 0; i < count; ++i) rows[i] = matches[(size_t)i].row;
    return FS_OK;
}

}  // extern "C"
