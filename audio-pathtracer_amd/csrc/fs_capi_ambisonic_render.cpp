// fs_capi_ambisonic_render.cpp — ambisonic voices on the audio thread: the encoder for hosts that put other beds into the same
// bus (fs_ambisonic_encode, host only), and what the renderer is beyond its voice bank (fs_capi_voice_bank.hpp: the callback;
// fs_capi_reflect_render.cpp: the set-up and its release): the order a source was initialised with — one per call — an entry's
// gain and direction, a state block with 128-byte slots and ONE history ring, and rows of C = (order + 1)^2 channels.  The band
// kernels and their per-context cache are the direct renderer's (fs_capi_direct_render.cpp).  The reference has no slot for it.
#include "fs_capi_voice_bank.hpp"

static_assert(sizeof(fs_ambisonic_voice) == 56, "fs_ambisonic_voice: the key, the delay, the bands, the gain, the direction");
static_assert(sizeof(fs_ambisonic_render_row) == 16, "fs_ambisonic_render_row: four counts");
static_assert((FS_MAX_AMBISONIC_ORDER + 1) * (FS_MAX_AMBISONIC_ORDER + 1) == kAmbisonicChannels, "the slot's and the plan's channel gains");

extern "C" {

int fs_ambisonic_encode(int32_t order, const float* direction, float* out) {
    if (order < 0 || order > FS_MAX_AMBISONIC_ORDER || !direction || !out || !ambisonic_direction_ok(direction)) return FS_ERR_INVALID_ARGUMENT;
    float y[kAmbisonicChannels];
    ambisonic_encode(order, direction, y);
    std::memcpy(out, y, sizeof(float) * (size_t)((order + 1) * (order + 1)));
    return FS_OK;
}

int fs_ambisonic_render_init(fs_context* ctx, fs_source h, int32_t frame_size, int32_t taps, int32_t voices, float max_delay_seconds,
                             int32_t order) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (order < 0 || order > FS_MAX_AMBISONIC_ORDER)   // (before the set-up: a refused init leaves the source as it was)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_ambisonic_render_init: order outside 0 .. FS_MAX_AMBISONIC_ORDER");
    // (no set to miss, and taps <= 2047 alone cannot be too many)
    const int rc = voice_bank_init(ctx, h, &Source::ar, 0,
                                   {nullptr, "fs_ambisonic_render_init: frame size outside 16 .. 16384, taps even or outside 1 .. 2047, voices outside 1 .. 32, or a bad max delay",
                                    nullptr, "fs_ambisonic_render_init: max delay + taps + 1 + frame size exceed 1 048 576 samples"},
                                   frame_size, taps, voices, max_delay_seconds, kAmbisonicBankHeader, 1);
    if (rc == FS_OK) s->ar.order = order;
    return rc;
}

int fs_ambisonic_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    return voice_bank_release(ctx, h, &Source::ar, kAmbisonicBankHeader, 1);
}

int fs_ambisonic_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                                      const fs_ambisonic_voice* voices, const int32_t* voice_counts, int32_t stride, float* out,
                                      float* mix, fs_ambisonic_render_row* rows) {
    static const VoiceBankRenderer<AmbisonicRenderBatch> q = {&Source::ar, &fs_context::ar_stage, "fs_ambisonic_render_init has not been called for this source",
                                                              nullptr, launch_ambisonic_render, kAmbisonicBankHeader};
    int order = -1;   // row 0's, which the others share
    return voice_bank_process(
        q, ctx, sources, count, in, voices, voice_counts, stride, out, mix, rows,
        [&](const fs_ambisonic_voice& v) {
            if (!std::isfinite(v.gain)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's gain is not finite");
            if (!ambisonic_direction_ok(v.direction))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's direction is not finite, or its squared length lies outside 1e-30 .. 1e30");
            return (int)FS_OK;
        },
        [&](const VoiceBank& bank) {
            if (order < 0) order = bank.order;
            if (bank.order != order) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "the sources of a batch share one ambisonic order");
            return (int)FS_OK;
        },
        [&](size_t, const RenderSetup& shape) {
            return std::array<size_t, 3>{0, 0, (size_t)((order + 1) * (order + 1)) * (size_t)shape.frame};
        },
        [&](AmbisonicRenderBatch& b, AmbisonicRenderItem*, char*, char*, char*) { b.order = order; });
}

}  // extern "C"
