// fs_capi_binaural_render.cpp — binaural voices on the audio thread: the HRIR set of the context (fs_hrtf_set / fs_hrtf_info), a
// set for hosts that have none (fs_hrtf_spherical_head, host only), and what the renderer is beyond its voice bank
// (fs_capi_voice_bank.hpp: the callback; fs_capi_reflect_render.cpp: the set-up and its release): the refusals that name the
// set, an entry's gain and direction, the list of sounding slots and the folded tables of fs_binaural_render.hip's launches.
// The band kernels and their per-context cache are the direct renderer's (fs_capi_direct_render.cpp).  The reference has no slot
// for it.
#include "fs_capi_voice_bank.hpp"

static_assert(sizeof(fs_binaural_voice) == 56, "fs_binaural_voice: the key, the delay, the bands, the gain, the direction");
static_assert(sizeof(fs_binaural_render_row) == 16, "fs_binaural_render_row: four counts");
static_assert(FS_MAX_REFLECTION_RENDER_BATCH * FS_MAX_REFLECTION_VOICES <= 65536, "BinauralRenderBatch::sounding: 16 bits per (row, slot)");

namespace {

constexpr double kPi = 3.14159265358979323846;

// the header's spherical-head model for one ear at angle theta from the ear's axis, in double: h[0 .. H)
void head_taps(double theta, double a_over_c, double fs, int H, double* h) {
    const double tau = theta <= kPi / 2.0 ? a_over_c * (1.0 - std::cos(theta)) : a_over_c * (1.0 + theta - kPi / 2.0);
    const double alpha_min = 0.1, theta_min = 5.0 * kPi / 6.0;
    const double alpha = (1.0 + alpha_min / 2.0) + (1.0 - alpha_min / 2.0) * std::cos(theta * kPi / theta_min);
    const double kappa = fs * a_over_c;
    const double b0 = (1.0 + alpha * kappa) / (1.0 + kappa), b1 = (1.0 - alpha * kappa) / (1.0 + kappa), a1 = (1.0 - kappa) / (1.0 + kappa);
    const double pos = tau * fs;
    const double fl = std::floor(pos);
    const int i = (int)fl;
    const double f = pos - fl;
    // g[m], m = k - i, and g[m - 1], walked along with k
    double g_prev = 0.0, g = 0.0;
    for (int k = 0; k < H; ++k) {
        const int m = k - i;
        g_prev = g;
        if (m < 0) g = 0.0;
        else if (m == 0) g = b0;
        else if (m == 1) g = b1 - a1 * g_prev;
        else g = -a1 * g_prev;
        h[k] = (1.0 - f) * g + f * g_prev;
    }
}

}  // namespace

extern "C" {

int fs_hrtf_spherical_head(int32_t sample_rate, float radius_cm, float sound_speed_cm_s, int32_t directions, int32_t taps, float* dirs,
                           float* hrir) {
    if (!dirs || !hrir || sample_rate < 1 || !std::isfinite(radius_cm) || !(radius_cm > 0.0f) || !std::isfinite(sound_speed_cm_s) ||
        !(sound_speed_cm_s > 0.0f) || directions < 1 || directions > FS_MAX_HRTF_DIRECTIONS || taps < 1 || taps > FS_MAX_HRTF_TAPS)
        return FS_ERR_INVALID_ARGUMENT;
    const double fs = (double)sample_rate, a_over_c = (double)radius_cm / (double)sound_speed_cm_s;
    if ((double)taps < std::ceil(a_over_c * (1.0 + kPi / 2.0) * fs) + 2.0) return FS_ERR_INVALID_ARGUMENT;
    const int n = directions, H = taps;
    std::vector<double> h((size_t)H);
    for (int k = 0; k < n; ++k) {
        const double z = 1.0 - (2.0 * (double)k + 1.0) / (double)n;
        const double rho = std::sqrt(1.0 - z * z);
        const double phi = (double)k * kPi * (3.0 - std::sqrt(5.0));
        const double p[3] = {rho * std::cos(phi), rho * std::sin(phi), z};
        for (int c = 0; c < 3; ++c) dirs[(size_t)k * 3 + c] = (float)p[c];
        for (int ear = 0; ear < 2; ++ear) {
            const double dot = ear == 0 ? -p[1] : p[1];   // p . e, e = (0, -+1, 0)
            const double theta = std::acos(std::min(std::max(dot, -1.0), 1.0));
            head_taps(theta, a_over_c, fs, H, h.data());
            float* out = hrir + ((size_t)k * 2 + (size_t)ear) * (size_t)H;
            for (int t = 0; t < H; ++t) out[t] = (float)h[(size_t)t];
        }
    }
    return FS_OK;
}

int fs_hrtf_set(fs_context* ctx, const fs_hrtf_desc* d) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    size_t n_dir = 0, n_tap = 0;
    if (d) {
        if (d->struct_size != sizeof(fs_hrtf_desc)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_desc.struct_size mismatch");
        if (d->directions < 1 || d->directions > FS_MAX_HRTF_DIRECTIONS || d->taps < 1 || d->taps > FS_MAX_HRTF_TAPS || !d->dirs || !d->hrir)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set: directions outside 1 .. 4096, taps outside 1 .. 512, or a NULL array");
        if (d->sample_rate != ctx->cfg.sample_rate)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set: the set's sample rate is not the context's");
        n_dir = (size_t)d->directions * 3;
        n_tap = (size_t)d->directions * 2 * (size_t)d->taps;
        for (int32_t j = 0; j < d->directions; ++j) {
            const float* p = d->dirs + (size_t)j * 3;
            const double len2 = (double)p[0] * (double)p[0] + (double)p[1] * (double)p[1] + (double)p[2] * (double)p[2];
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !(std::fabs(len2 - 1.0) <= 1e-3))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set: a direction is not finite or not a unit vector");
        }
        for (size_t t = 0; t < n_tap; ++t)
            if (!std::isfinite(d->hrir[t])) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set: a tap is not finite");
    }
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    float* fresh = nullptr;
    if (d) FS_HIP(ctx, hipMalloc((void**)&fresh, sizeof(float) * (n_dir + n_tap)));   // (a failure here has changed nothing)
    hipError_t err = hipStreamSynchronize(ctx->rev_stream);   // no callback reads the old set any more
    if (err == hipSuccess && d) {
        std::vector<float> both(n_dir + n_tap);   // dirs | hrir: one copy
        std::memcpy(both.data(), d->dirs, sizeof(float) * n_dir);
        std::memcpy(both.data() + n_dir, d->hrir, sizeof(float) * n_tap);
        err = hipMemcpy(fresh, both.data(), sizeof(float) * both.size(), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) { if (fresh) (void)hipFree(fresh); return ctx->hip_fail(err, "fs_hrtf_set (upload)"); }
    if (ctx->d_hrtf) (void)hipFree(ctx->d_hrtf);
    ctx->d_hrtf = fresh;
    ctx->hrtf_dirs = d ? d->directions : 0;
    ctx->hrtf_taps = d ? d->taps : 0;
    // Every held slot is free, on both copies of the slot tables; the rings and the counters stay.  The set is in force from here
    // on, so no source is left out: the host's copies — what the matching reads, so every voice starts — all go first, and a
    // failed clear of a device copy (which a start overwrites anyway) is reported only after every source has had its turn.
    for (Source* s : ctx->sources)
        if (s && s->alive && s->br.r.d) s->br.free_slots();
    hipError_t clear_err = hipSuccess;
    for (Source* s : ctx->sources) {
        if (!s || !s->alive || !s->br.r.d) continue;
        const hipError_t e = hipMemsetAsync(s->br.r.d + offsetof(BinauralRenderState, slot), 0, sizeof(BinauralRenderState::slot), ctx->rev_stream);
        if (e != hipSuccess && clear_err == hipSuccess) clear_err = e;
    }
    if (clear_err != hipSuccess) return ctx->hip_fail(clear_err, "fs_hrtf_set (clearing the slots)");
    return FS_OK;
}

int fs_hrtf_info(fs_context* ctx, int32_t* directions, int32_t* taps) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (directions) *directions = ctx->hrtf_dirs;
    if (taps) *taps = ctx->hrtf_taps;
    return FS_OK;
}

int fs_binaural_render_init(fs_context* ctx, fs_source h, int32_t frame_size, int32_t taps, int32_t voices, float max_delay_seconds) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    return voice_bank_init(ctx, h, &Source::br, ctx->hrtf_dirs ? ctx->hrtf_taps - 1 : -1,
                           {"fs_binaural_render_init: no HRIR set in force (fs_hrtf_set)",
                            "fs_binaural_render_init: frame size outside 16 .. 16384, taps even or outside 1 .. 2047, voices outside 1 .. 32, or a bad max delay",
                            "fs_binaural_render_init: taps + the set's taps - 1 exceed 2047",
                            "fs_binaural_render_init: max delay + folded taps + 1 + frame size exceed 1 048 576 samples"},
                           frame_size, taps, voices, max_delay_seconds, kVoiceBankHeader, 2);
}

int fs_binaural_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    return voice_bank_release(ctx, h, &Source::br, kVoiceBankHeader, 2);
}

int fs_binaural_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                                     const fs_binaural_voice* voices, const int32_t* voice_counts, int32_t stride, float* out,
                                     float* mix, fs_binaural_render_row* rows) {
    static const VoiceBankRenderer<BinauralRenderBatch> q = {&Source::br, &fs_context::br_stage, "fs_binaural_render_init has not been called for this source",
                                                             "fs_binaural_render_process_batch: no HRIR set in force (fs_hrtf_set)", launch_binaural_render, kVoiceBankHeader};
    const int H = ctx ? ctx->hrtf_taps : 0;
    return voice_bank_process(
        q, ctx, sources, count, in, voices, voice_counts, stride, out, mix, rows,
        [&](const fs_binaural_voice& v) {
            if (!std::isfinite(v.gain)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's gain is not finite");
            const float* dir = v.direction;
            if (!std::isfinite(dir[0]) || !std::isfinite(dir[1]) || !std::isfinite(dir[2]) || (dir[0] == 0.0f && dir[1] == 0.0f && dir[2] == 0.0f))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's direction is not finite or is the zero vector");
            return (int)FS_OK;
        },
        [&](const VoiceBank& bank) {
            const int tc = bank.r.taps + H - 1;
            if (tc > FS_DIRECT_RENDER_MAX_TAPS || (double)bank.r.max_delay + (double)tc + 1.0 + (double)bank.r.frame > (double)bank.r.ring)
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "the HRIR set in force has outgrown this source's history: call fs_binaural_render_init again");
            return (int)FS_OK;
        },
        // the sounding slots' list | the folded tables (sized by the rows' slots, not by how many sound in this call: a shape
        // allocates once)
        [&](size_t slots, const RenderSetup& shape) {
            return std::array<size_t, 3>{sizeof(uint16_t) * slots, sizeof(float2) * slots * 2 * (size_t)(shape.taps + H - 1), 2 * (size_t)shape.frame};
        },
        [&](BinauralRenderBatch& b, BinauralRenderItem* items, char* h_sounding, char* d_sounding, char* d_folded) {
            uint16_t* sounding = (uint16_t*)h_sounding;
            for (int i = 0; i < b.count; ++i) {
                items[i].first = b.n_sounding;
                for (int j = 0; j < items[i].slots; ++j)
                    if (items[i].op[j] != kVoiceIdle) sounding[b.n_sounding++] = (uint16_t)(i * kVoiceSlots + j);
            }
            b.sounding = (const uint16_t*)d_sounding;
            b.folded = (float2*)d_folded;
            b.dirs = ctx->d_hrtf;
            b.hrir = ctx->d_hrtf + (size_t)ctx->hrtf_dirs * 3;
            b.n_dirs = ctx->hrtf_dirs; b.h_taps = H;
            b.tc = b.taps + H - 1;
        });
}

}  // extern "C"
