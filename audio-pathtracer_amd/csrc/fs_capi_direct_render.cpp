// fs_capi_direct_render.cpp — the direct sound on the audio thread: the band kernels (fs_direct_band_kernels, host only), the
// per-source set-up (fs_direct_render_init / _release) and the callback of all sources (fs_direct_render_process_batch: one copy
// up, the launches of fs_direct_render.hip, one copy back, one wait).  The reference's slot for it is
// FFrequenSeeAudioOcclusionPlugin::ProcessAudio, which leaves the multiply commented out.
#include "fs_context.hpp"

static_assert(sizeof(fs_direct_render_target) == 36, "fs_direct_render_target: the delay and the bands");

namespace {

constexpr double kPi = 3.14159265358979323846;

// the inner edges in force for B bands: the ones given, else the default octave edges
std::vector<double> inner_edges(const std::vector<double>& given, int B) {
    if (!given.empty()) return given;
    std::vector<double> e;
    for (int b = 1; b < B; ++b) e.push_back(125.0 * std::pow(2.0, (double)b - 0.5));
    return e;
}

bool edges_fit(const std::vector<double>& e, int sample_rate) {
    for (size_t i = 0; i < e.size(); ++i)
        if (!std::isfinite(e[i]) || !(e[i] > 0.0) || !(e[i] < (double)sample_rate / 2.0) || (i > 0 && !(e[i] > e[i - 1]))) return false;
    return true;
}

// k_b[t] = w[m] (L_{e_{b+1}}[m] - L_{e_b}[m]) in double, rounded to float once; e = the B - 1 inner edges (checked by the caller)
void band_kernels(int sample_rate, const std::vector<double>& e, int B, int T, float* out) {
    const double fs = (double)sample_rate;
    const int c = (T - 1) / 2;
    auto lowpass = [&](int edge, int m) -> double {   // edge 0 .. B
        if (edge == 0) return 0.0;
        if (edge == B) return m == 0 ? 1.0 : 0.0;   // Nyquist: the unit impulse, taken exactly
        const double f = e[(size_t)edge - 1];
        if (m == 0) return 2.0 * f / fs;
        return std::sin(2.0 * kPi * f * (double)m / fs) / (kPi * (double)m);
    };
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            const int m = t - c;
            const double w = 0.5 + 0.5 * std::cos(kPi * (double)m / (double)(c + 1));
            out[(size_t)b * (size_t)T + t] = (float)(w * (lowpass(b + 1, m) - lowpass(b, m)));
        }
}

bool taps_ok(int32_t taps) { return direct_render_taps_ok(taps); }

}  // namespace

namespace fsi {

bool direct_render_taps_ok(int32_t taps) { return taps >= 1 && taps <= FS_DIRECT_RENDER_MAX_TAPS && (taps & 1) == 1; }

int direct_render_table_for(fs_context* ctx, int taps, const float** out) {
    const int B = ctx->cfg.num_bands;
    const std::vector<double> e = inner_edges(ctx->band_edges, B);
    for (const auto& t : ctx->dr_tables)
        if (t.taps == taps && t.edges == e) { *out = t.d; return FS_OK; }
    if (!edges_fit(e, ctx->cfg.sample_rate))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_direct_render_init: the band edges in force do not lie in (0, sample_rate / 2): give edges with fs_set_band_edges");
    std::vector<float> k((size_t)B * (size_t)taps);
    band_kernels(ctx->cfg.sample_rate, e, B, taps, k.data());
    float* d = nullptr;
    FS_HIP(ctx, hipMalloc((void**)&d, sizeof(float) * k.size()));
    const hipError_t err = hipMemcpy(d, k.data(), sizeof(float) * k.size(), hipMemcpyHostToDevice);
    if (err != hipSuccess) { (void)hipFree(d); return ctx->hip_fail(err, "hipMemcpy (band kernels)"); }
    ctx->dr_tables.push_back({taps, e, d});
    *out = d;
    return FS_OK;
}

int render_setup(fs_context* ctx, RenderSetup& r, size_t header, int rings, int frame, int taps, double d_max, double need) {
    unsigned ring = 1;
    while ((double)ring < need) ring <<= 1;
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const float* table = nullptr;
    const int rc = direct_render_table_for(ctx, taps, &table);
    if (rc) return rc;
    FS_HIP(ctx, hipStreamSynchronize(ctx->rev_stream));
    if (r.d) (void)hipFree(r.d);
    r = RenderSetup{nullptr, frame, taps, (int)d_max, ring, table};
    const size_t bytes = header + sizeof(float) * (size_t)rings * (size_t)ring;
    FS_HIP(ctx, hipMalloc((void**)&r.d, bytes));
    FS_HIP(ctx, hipMemsetAsync(r.d, 0, bytes, ctx->rev_stream));
    return FS_OK;
}

int render_clear(fs_context* ctx, const RenderSetup& r, size_t header, int rings) {
    if (r.d && ctx->device_ok) {
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        FS_HIP(ctx, hipMemsetAsync(r.d, 0, header + sizeof(float) * (size_t)rings * (size_t)r.ring, ctx->rev_stream));
    }
    return FS_OK;
}

int render_aim_check(fs_context* ctx, const char* whose, float delay, const float* band_gain, const RenderSetup& r) {
    if (!std::isfinite(delay) || !(delay >= 0.0f) || delay * (float)ctx->cfg.sample_rate > (float)r.max_delay)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, std::string("a ") + whose + "'s delay is negative, not finite or beyond the source's max delay");
    for (int b = 0; b < ctx->cfg.num_bands; ++b)
        if (!std::isfinite(band_gain[b]) || !(band_gain[b] >= 0.0f))
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, std::string("a ") + whose + "'s band gain is negative or not finite");
    return FS_OK;
}

int render_no_duplicates(fs_context* ctx, const std::vector<Source*>& srcs) {
    std::vector<Source*> sorted(srcs);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a source appears twice in the batch");
    return FS_OK;
}

}  // namespace fsi

extern "C" {

int fs_direct_band_kernels(int32_t sample_rate, const float* edges_hz, int32_t bands, int32_t taps, float* out) {
    if (!out || bands < 1 || bands > FS_MAX_BANDS || !taps_ok(taps) || sample_rate < 1) return FS_ERR_INVALID_ARGUMENT;
    std::vector<double> given;
    if (edges_hz)
        for (int b = 0; b + 1 < bands; ++b) given.push_back((double)edges_hz[b]);
    const std::vector<double> e = edges_hz ? given : inner_edges(given, bands);
    if (!edges_fit(e, sample_rate)) return FS_ERR_INVALID_ARGUMENT;
    band_kernels(sample_rate, e, bands, taps, out);
    return FS_OK;
}

int fs_direct_render_init(fs_context* ctx, fs_source h, int32_t frame_size, int32_t taps, float max_delay_seconds) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (frame_size < 16 || frame_size > 16384 || !taps_ok(taps) || !std::isfinite(max_delay_seconds) || !(max_delay_seconds >= 0.0f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_direct_render_init: frame size outside 16 .. 16384, taps even or outside 1 .. 2047, or a bad max delay");
    const double d_max = std::ceil((double)max_delay_seconds * (double)ctx->cfg.sample_rate);
    const double need = d_max + (double)taps + 1.0 + (double)frame_size;
    if (need > 1048576.0)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_direct_render_init: max delay + taps + 1 + frame size exceed 1 048 576 samples");
    return render_setup(ctx, s->dr, kDirectRenderHeader, 2, frame_size, taps, d_max, need);
}

int fs_direct_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    return render_clear(ctx, s->dr, kDirectRenderHeader, 2);   // history := 0, not primed
}

int fs_direct_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                                   const fs_direct_render_target* targets, float* out, float* mix) {
    if (!ctx || !sources || !in || !targets || (!out && !mix)) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (count < 1 || count > FS_MAX_DIRECT_RENDER_BATCH)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_DIRECT_RENDER_BATCH)");
    // Everything is validated before the first state change or enqueue: a refused call changes nothing.
    const int B = ctx->cfg.num_bands;
    const float fs_f = (float)ctx->cfg.sample_rate;
    std::vector<Source*> srcs((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        int rc;
        srcs[(size_t)i] = render_row(ctx, sources[i], [](const Source& s) -> const RenderSetup& { return s.dr; }, "fs_direct_render_init has not been called for this source", i ? srcs[0] : nullptr, &rc);
        if (!rc) rc = render_aim_check(ctx, "target", targets[i].delay, targets[i].band_gain, srcs[(size_t)i]->dr);
        if (rc) return rc;
    }
    { const int rc = render_no_duplicates(ctx, srcs); if (rc) return rc; }
    const int frame = srcs[0]->dr.frame;
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const CallbackLayout l = callback_layout(count, frame, 2 * (size_t)frame, {sizeof(DirectRenderItem) * (size_t)count}, {sizeof(DirectRenderPlan) * (size_t)count});
    { const int rc = ctx->dr_stage.fit(ctx, l.host_bytes, l.dev_bytes); if (rc) return rc; }
    char* hs = ctx->dr_stage.h; char* ds = ctx->dr_stage.d;
    DirectRenderItem* items = (DirectRenderItem*)(hs + l.up[0]);
    for (int32_t i = 0; i < count; ++i) {
        const RenderSetup& r = srcs[(size_t)i]->dr;
        DirectRenderItem& it = items[i];
        std::memset(&it, 0, sizeof(it));
        it.state = (DirectRenderState*)r.d;
        it.ring = (float*)(r.d + kDirectRenderHeader);
        it.table = r.table;
        it.mask = r.ring - 1u;
        it.d1 = targets[i].delay * fs_f;
        for (int b = 0; b < B; ++b) it.g1[b] = targets[i].band_gain[b];
    }
    std::memcpy(hs + l.in, in, l.in_rows);
    FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, ctx->rev_stream));
    DirectRenderBatch b{};
    b.items = (const DirectRenderItem*)(ds + l.up[0]);
    b.plans = (DirectRenderPlan*)(ds + l.scratch[0]);
    b.count = count; b.frame = frame; b.taps = srcs[0]->dr.taps; b.bands = B;
    b.in = (const float*)(ds + l.in);
    b.out = (float*)(ds + l.d_out);
    b.mix = mix ? (float*)(ds + l.d_mix) : nullptr;
    launch_direct_render(b, ctx->rev_stream);
    FS_HIP(ctx, hipGetLastError());
    { const int rc = callback_finish(ctx, ctx->dr_stage, l, out != nullptr, mix); if (rc) return rc; }
    if (out) std::memcpy(out, hs + l.h_out, l.rows);
    return FS_OK;
}

}  // extern "C"
