// fs_capi_reflect_render.cpp — the early reflections on the audio thread, and the host side of the voice bank they and the
// binaural voices (fs_capi_binaural_render.cpp) are built on: the matching of a row's entries to the slots (voice_match), the
// per-source set-up and its release (voice_bank_init / _release, behind fs_reflection_render_init / _release,
// fs_binaural_render_init / _release and fs_ambisonic_render_init / _release).  The callback of all sources, fs_reflection_render_process_batch, is
// fs_capi_voice_bank.hpp's voice_bank_process with the channel gains as an entry's own fields and fs_reflect_render.hip's
// launches.  The band kernels and their per-context cache are the direct renderer's (fs_capi_direct_render.cpp).  The reference
// has no slot for it.
#include "fs_capi_voice_bank.hpp"

static_assert(sizeof(fs_reflection_voice) == 48, "fs_reflection_voice: the key, the delay, the bands, two channels");
static_assert(sizeof(fs_reflection_render_row) == 16, "fs_reflection_render_row: four counts");

namespace fsi {

// Rule 1 of the header: held slots continue or end by their key; the other entries start, in list order, on the lowest slot that
// was free when the callback began; what finds none is dropped.  (n entries with distinct keys: checked by the caller.)
VoiceMatch voice_match(const VoiceBank& bank, const void* voices, size_t voice_bytes, int n) {
    const int V = bank.voices;
    VoiceMatch m{};
    auto key_of = [&](int e) { uint32_t k; std::memcpy(&k, (const char*)voices + (size_t)e * voice_bytes, sizeof(k)); return k; };
    bool taken[FS_MAX_REFLECTION_VOICES] = {};   // entries a held slot continues with
    for (int j = 0; j < FS_MAX_REFLECTION_VOICES; ++j) m.op[j] = (int8_t)kVoiceIdle;
    for (int j = 0; j < V; ++j) {
        if (!bank.held[j]) continue;
        int e = 0;
        while (e < n && key_of(e) != bank.key[j]) ++e;
        if (e < n) {
            m.op[j] = (int8_t)(kVoiceContinue + e);
            m.held[j] = true; m.key[j] = bank.key[j];
            taken[e] = true;
        } else {
            m.op[j] = (int8_t)kVoiceEnd;
            m.row.ended++;
        }
        m.row.sounding++;
    }
    int next = 0;   // the lowest slot not looked at yet
    for (int e = 0; e < n; ++e) {
        if (taken[e]) continue;
        while (next < V && bank.held[next]) ++next;  // (an ending slot is held during this callback)
        if (next == V) { m.row.dropped++; continue; }
        m.op[next] = (int8_t)(kVoiceStart + e);
        m.held[next] = true; m.key[next] = key_of(e);
        m.row.started++; m.row.sounding++;
        ++next;
    }
    return m;
}

int voice_bank_init(fs_context* ctx, fs_source h, VoiceBank Source::*which, int fold_taps, const VoiceBankInitTexts& t, int32_t frame_size,
                    int32_t taps, int32_t voices, float max_delay_seconds, size_t header, int rings) {
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (fold_taps < 0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, t.no_set);
    if (frame_size < 16 || frame_size > 16384 || !direct_render_taps_ok(taps) || voices < 1 || voices > FS_MAX_REFLECTION_VOICES ||
        !std::isfinite(max_delay_seconds) || !(max_delay_seconds >= 0.0f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, t.ranges);
    const int tc = taps + fold_taps;   // the taps the history serves
    if (tc > FS_DIRECT_RENDER_MAX_TAPS) return ctx->fail(FS_ERR_INVALID_ARGUMENT, t.folded);
    const double d_max = std::ceil((double)max_delay_seconds * (double)ctx->cfg.sample_rate);
    const double need = d_max + (double)tc + 1.0 + (double)frame_size;
    if (need > 1048576.0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, t.ring);
    VoiceBank& bank = s->*which;
    const int rc = render_setup(ctx, bank.r, header, rings, frame_size, taps, d_max, need);
    if (rc) return rc;   // (without a set-up, or with the old one untouched)
    bank.voices = voices;
    bank.free_slots();
    return FS_OK;
}

int voice_bank_release(fs_context* ctx, fs_source h, VoiceBank Source::*which, size_t header, int rings) {
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    const int rc = render_clear(ctx, (s->*which).r, header, rings);   // history := 0 ...
    if (rc == FS_OK) (s->*which).free_slots();                            // ... every slot free
    return rc;
}

}  // namespace fsi

extern "C" {

int fs_reflection_render_init(fs_context* ctx, fs_source h, int32_t frame_size, int32_t taps, int32_t voices, float max_delay_seconds) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    // (no set to miss, and taps <= 2047 alone cannot be too many)
    return voice_bank_init(ctx, h, &Source::rr, 0,
                           {nullptr, "fs_reflection_render_init: frame size outside 16 .. 16384, taps even or outside 1 .. 2047, voices outside 1 .. 32, or a bad max delay",
                            nullptr, "fs_reflection_render_init: max delay + taps + 1 + frame size exceed 1 048 576 samples"},
                           frame_size, taps, voices, max_delay_seconds, kVoiceBankHeader, 2);
}

int fs_reflection_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    return voice_bank_release(ctx, h, &Source::rr, kVoiceBankHeader, 2);
}

int fs_reflection_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                                       const fs_reflection_voice* voices, const int32_t* voice_counts, int32_t stride, float* out,
                                       float* mix, fs_reflection_render_row* rows) {
    static const VoiceBankRenderer<ReflectRenderBatch> q = {&Source::rr, &fs_context::rr_stage, "fs_reflection_render_init has not been called for this source",
                                                            nullptr, launch_reflect_render, kVoiceBankHeader};
    return voice_bank_process(
        q, ctx, sources, count, in, voices, voice_counts, stride, out, mix, rows,
        [&](const fs_reflection_voice& v) {
            if (!std::isfinite(v.channel_gain[0]) || !std::isfinite(v.channel_gain[1]))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's channel gain is not finite");
            return (int)FS_OK;
        },
        [](const VoiceBank&) { return (int)FS_OK; }, [](size_t, const RenderSetup& shape) { return std::array<size_t, 3>{0, 0, 2 * (size_t)shape.frame}; },
        [](ReflectRenderBatch&, ReflectRenderItem*, char*, char*, char*) {});
}

}  // extern "C"
