// fs_capi_binaural_render.cpp — binaural voices on the audio thread: the HRIR set of the context (fs_hrtf_set / fs_hrtf_info), a
// set for hosts that have none (fs_hrtf_spherical_head, host only), the per-source set-up (fs_binaural_render_init / _release)
// and the callback of all sources (fs_binaural_render_process_batch: everything validated, the voices matched to the slots on
// the host's copy of the slot table by the reflection renderer's voice_match, one copy up, the launches of
// fs_binaural_render.hip, one copy back, one wait).  The band kernels and their per-context cache are the direct renderer's
// (fs_capi_direct_render.cpp).  The reference has no slot for it.
#include "fs_context.hpp"

static_assert(sizeof(fs_binaural_voice) == 56, "fs_binaural_voice: the key, the delay, the bands, the gain, the direction");
static_assert(sizeof(fs_binaural_render_row) == 16, "fs_binaural_render_row: four counts");
static_assert(FS_MAX_REFLECTION_RENDER_BATCH * FS_MAX_REFLECTION_VOICES <= 65536, "BinauralRenderBatch::sounding: 16 bits per (row, slot)");

namespace {

constexpr double kPi = 3.14159265358979323846;

void br_free_slots(Source* s) {
    for (int j = 0; j < FS_MAX_REFLECTION_VOICES; ++j) { s->br_held[j] = false; s->br_key[j] = 0; }
}

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
        if (s && s->alive && s->br.d) br_free_slots(s);
    hipError_t clear_err = hipSuccess;
    for (Source* s : ctx->sources) {
        if (!s || !s->alive || !s->br.d) continue;
        const hipError_t e = hipMemsetAsync(s->br.d + offsetof(BinauralRenderState, slot), 0, sizeof(BinauralRenderState::slot), ctx->rev_stream);
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
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (ctx->hrtf_dirs == 0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_binaural_render_init: no HRIR set in force (fs_hrtf_set)");
    if (frame_size < 16 || frame_size > 16384 || !direct_render_taps_ok(taps) || voices < 1 || voices > FS_MAX_REFLECTION_VOICES ||
        !std::isfinite(max_delay_seconds) || !(max_delay_seconds >= 0.0f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_binaural_render_init: frame size outside 16 .. 16384, taps even or outside 1 .. 2047, voices outside 1 .. 32, or a bad max delay");
    const int tc = taps + ctx->hrtf_taps - 1;
    if (tc > FS_DIRECT_RENDER_MAX_TAPS)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_binaural_render_init: taps + the set's taps - 1 exceed 2047");
    const double d_max = std::ceil((double)max_delay_seconds * (double)ctx->cfg.sample_rate);
    const double need = d_max + (double)tc + 1.0 + (double)frame_size;
    if (need > 1048576.0)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_binaural_render_init: max delay + folded taps + 1 + frame size exceed 1 048 576 samples");
    const int rc = render_setup(ctx, s->br, kBinauralRenderHeader, frame_size, taps, d_max, need);
    if (rc) return rc;   // (without a set-up, or with the old one untouched)
    s->br_voices = voices;
    br_free_slots(s);
    return FS_OK;
}

int fs_binaural_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    const int rc = render_clear(ctx, s->br, kBinauralRenderHeader);   // history := 0 ...
    if (rc == FS_OK) br_free_slots(s);                                 // ... every slot free
    return rc;
}

int fs_binaural_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                                     const fs_binaural_voice* voices, const int32_t* voice_counts, int32_t stride, float* out,
                                     float* mix, fs_binaural_render_row* rows) {
    if (!ctx || !sources || !in || !voices || !voice_counts || (!out && !mix)) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (count < 1 || count > FS_MAX_REFLECTION_RENDER_BATCH)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REFLECTION_RENDER_BATCH)");
    if (stride < 1 || stride > FS_MAX_REFLECTION_VOICES)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "stride out of range (1 .. FS_MAX_REFLECTION_VOICES)");
    if (ctx->hrtf_dirs == 0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_binaural_render_process_batch: no HRIR set in force (fs_hrtf_set)");
    // Everything is validated before the first state change or enqueue: a refused call changes nothing.
    const int B = ctx->cfg.num_bands;
    const int H = ctx->hrtf_taps;
    const float fs_f = (float)ctx->cfg.sample_rate;
    std::vector<Source*> srcs((size_t)count);
    size_t slots_total = 0;
    for (int32_t i = 0; i < count; ++i) {
        int rc;
        Source* s = srcs[(size_t)i] = render_row(ctx, sources[i], &Source::br, "fs_binaural_render_init has not been called for this source", i ? srcs[0] : nullptr, &rc);
        if (rc) return rc;
        const int tc = s->br.taps + H - 1;
        if (tc > FS_DIRECT_RENDER_MAX_TAPS || (double)s->br.max_delay + (double)tc + 1.0 + (double)s->br.frame > (double)s->br.ring)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "the HRIR set in force has outgrown this source's history: call fs_binaural_render_init again");
        slots_total += (size_t)s->br_voices;
        const int32_t n = voice_counts[i];
        if (n < 0 || n > stride) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice count outside 0 .. stride");
        const fs_binaural_voice* v = voices + (size_t)i * (size_t)stride;
        for (int32_t e = 0; e < n; ++e) {
            for (int32_t f = 0; f < e; ++f)
                if (v[f].key == v[e].key) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a key appears twice in one row");
            rc = render_aim_check(ctx, "voice", v[e].delay, v[e].band_gain, s->br);
            if (rc) return rc;
            if (!std::isfinite(v[e].gain)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's gain is not finite");
            const float* dir = v[e].direction;
            if (!std::isfinite(dir[0]) || !std::isfinite(dir[1]) || !std::isfinite(dir[2]) || (dir[0] == 0.0f && dir[1] == 0.0f && dir[2] == 0.0f))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice's direction is not finite or is the zero vector");
        }
    }
    { const int rc = render_no_duplicates(ctx, srcs); if (rc) return rc; }
    const int frame = srcs[0]->br.frame, taps = srcs[0]->br.taps, tc = taps + H - 1;
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    enum { kItems, kVoices, kSounding, kN0 = 0, kPlans, kFolded };   // CallbackLayout::up and ::scratch
    // (the list and the folded tables are sized by the rows' slots, not by how many sound in this call: a shape allocates once)
    const CallbackLayout l = callback_layout(count, frame,
                                             {sizeof(BinauralRenderItem) * (size_t)count, sizeof(fs_binaural_voice) * (size_t)count * (size_t)stride,
                                              sizeof(uint16_t) * slots_total},
                                             {sizeof(unsigned) * (size_t)count, sizeof(BinauralRenderPlan) * (size_t)count * FS_MAX_REFLECTION_VOICES,
                                              sizeof(float2) * slots_total * 2 * (size_t)tc});
    { const int rc = ctx->br_stage.fit(ctx, l.host_bytes, l.dev_bytes); if (rc) return rc; }
    char* hs = ctx->br_stage.h; char* ds = ctx->br_stage.d;
    BinauralRenderItem* items = (BinauralRenderItem*)(hs + l.up[kItems]);
    uint16_t* sounding = (uint16_t*)(hs + l.up[kSounding]);
    int n_sounding = 0;
    std::vector<VoiceMatch> matches((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = srcs[(size_t)i];
        VoiceMatch& m = matches[(size_t)i] = voice_match(s->br_held, s->br_key, s->br_voices, voices + (size_t)i * (size_t)stride, sizeof(fs_binaural_voice), voice_counts[i]);
        BinauralRenderItem& it = items[i];
        std::memset(&it, 0, sizeof(it));
        it.state = (BinauralRenderState*)s->br.d;
        it.ring = (float*)(s->br.d + kBinauralRenderHeader);
        it.table = s->br.table;
        it.mask = s->br.ring - 1u;
        it.slots = s->br_voices;
        std::memcpy(it.op, m.op, sizeof(it.op));
        it.first = n_sounding;
        for (int j = 0; j < s->br_voices; ++j)
            if (m.op[j] != kReflectIdle) sounding[n_sounding++] = (uint16_t)(i * FS_MAX_REFLECTION_VOICES + j);
    }
    std::memcpy(hs + l.up[kVoices], voices, sizeof(fs_binaural_voice) * (size_t)count * (size_t)stride);
    std::memcpy(hs + l.in, in, l.rows);
    FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
    BinauralRenderBatch b{};
    b.items = (const BinauralRenderItem*)(ds + l.up[kItems]);
    b.voices = (const fs_binaural_voice*)(ds + l.up[kVoices]);
    b.sounding = (const uint16_t*)(ds + l.up[kSounding]);
    b.plans = (BinauralRenderPlan*)(ds + l.scratch[kPlans]);
    b.n0 = (unsigned*)(ds + l.scratch[kN0]);
    b.folded = (float2*)(ds + l.scratch[kFolded]);
    b.dirs = ctx->d_hrtf;
    b.hrir = ctx->d_hrtf + (size_t)ctx->hrtf_dirs * 3;
    b.n_dirs = ctx->hrtf_dirs; b.h_taps = H;
    b.count = count; b.stride = stride; b.frame = frame; b.taps = taps; b.tc = tc; b.bands = B; b.n_sounding = n_sounding;
    b.fs = fs_f;
    b.in = (const float*)(ds + l.in);
    b.out = (float*)(ds + l.d_out);
    b.mix = mix ? (float*)(ds + l.d_mix) : nullptr;
    launch_binaural_render(b, rs);
    FS_HIP(ctx, hipGetLastError());
    for (int32_t i = 0; i < count; ++i) {   // the plan pass is on its way: the slot tables are what it leaves behind
        Source* s = srcs[(size_t)i];
        std::memcpy(s->br_held, matches[(size_t)i].held, sizeof(s->br_held));
        std::memcpy(s->br_key, matches[(size_t)i].key, sizeof(s->br_key));
    }
    { const int rc = callback_finish(ctx, ctx->br_stage, l, out != nullptr, mix); if (rc) return rc; }
    if (out) std::memcpy(out, hs + l.h_out, l.rows);
    if (rows)
        for (int32_t i = 0; i < count; ++i) {
            const fs_reflection_render_row& r = matches[(size_t)i].row;
            rows[i] = fs_binaural_render_row{r.sounding, r.started, r.ended, r.dropped};
        }
    return FS_OK;
}

}  // extern "C"
