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

// The staging of one callback (fs_context::h_dr_stage / d_dr_stage), every block 256-byte aligned
struct DrStageLayout {
    size_t items, in, up_bytes;              // host and device, the same offsets: what goes up in one copy
    size_t h_out, h_mix, host_bytes;         // host: what comes back
    size_t d_plans, d_out, d_mix, dev_bytes; // device: out | mix adjacent, one copy back
};
size_t dr_align(size_t b) { return (b + 255) & ~(size_t)255; }
DrStageLayout dr_stage_layout(int count, int frame) {
    const size_t rows = sizeof(float) * 2 * (size_t)frame * (size_t)count, row = sizeof(float) * 2 * (size_t)frame;
    DrStageLayout l;
    l.items = 0;
    l.in = dr_align(sizeof(DirectRenderItem) * (size_t)count);
    l.up_bytes = l.in + rows;
    l.h_out = dr_align(l.up_bytes);
    l.h_mix = l.h_out + rows;   // (adjacent to out)
    l.host_bytes = l.h_mix + row;
    l.d_plans = dr_align(l.up_bytes);
    l.d_out = l.d_plans + dr_align(sizeof(DirectRenderPlan) * (size_t)count);
    l.d_mix = l.d_out + rows;
    l.dev_bytes = l.d_mix + row;
    return l;
}

size_t dr_state_bytes(const Source* s) { return kDirectRenderHeader + sizeof(float) * 2 * (size_t)s->dr_ring; }

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
    unsigned ring = 1;
    while ((double)ring < need) ring <<= 1;
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const float* table = nullptr;
    const int rc = direct_render_table_for(ctx, taps, &table);
    if (rc) return rc;
    FS_HIP(ctx, hipStreamSynchronize(ctx->rev_stream));
    if (s->d_dr) (void)hipFree(s->d_dr);
    s->d_dr = nullptr;
    s->dr_frame = frame_size;
    s->dr_taps = taps;
    s->dr_max_delay = (int)d_max;
    s->dr_ring = ring;
    s->dr_table = table;
    FS_HIP(ctx, hipMalloc((void**)&s->d_dr, dr_state_bytes(s)));
    FS_HIP(ctx, hipMemsetAsync(s->d_dr, 0, dr_state_bytes(s), ctx->rev_stream));
    return FS_OK;
}

int fs_direct_render_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (s->d_dr && ctx->device_ok) {   // history := 0, not primed
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        FS_HIP(ctx, hipMemsetAsync(s->d_dr, 0, dr_state_bytes(s), ctx->rev_stream));
    }
    return FS_OK;
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
        Source* s = srcs[(size_t)i] = get_source(ctx, sources[i]);
        if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
        if (!s->d_dr) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_direct_render_init has not been called for this source");
        if (s->dr_frame != srcs[0]->dr_frame || s->dr_taps != srcs[0]->dr_taps)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "the sources of a batch share one frame size and one tap count");
        const fs_direct_render_target& t = targets[i];
        if (!std::isfinite(t.delay) || !(t.delay >= 0.0f) || t.delay * fs_f > (float)s->dr_max_delay)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a target's delay is negative, not finite or beyond the source's max delay");
        for (int b = 0; b < B; ++b)
            if (!std::isfinite(t.band_gain[b]) || !(t.band_gain[b] >= 0.0f))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a target's band gain is negative or not finite");
    }
    {
        std::vector<Source*> sorted(srcs);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a source appears twice in the batch");
    }
    const int frame = srcs[0]->dr_frame;
    const size_t row = 2 * (size_t)frame;   // floats
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    const DrStageLayout l = dr_stage_layout(count, frame);
    if (l.host_bytes > ctx->dr_stage_host || l.dev_bytes > ctx->dr_stage_dev) {   // first call of this size (every call ends synchronised: nothing reads the old one)
        if (ctx->h_dr_stage) (void)hipHostFree(ctx->h_dr_stage);
        if (ctx->d_dr_stage) (void)hipFree(ctx->d_dr_stage);
        ctx->h_dr_stage = ctx->d_dr_stage = nullptr; ctx->dr_stage_host = ctx->dr_stage_dev = 0;
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_dr_stage, l.host_bytes, hipHostMallocDefault));
        ctx->dr_stage_host = l.host_bytes;
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_dr_stage, l.dev_bytes));
        ctx->dr_stage_dev = l.dev_bytes;
    }
    char* hs = ctx->h_dr_stage; char* ds = ctx->d_dr_stage;
    DirectRenderItem* items = (DirectRenderItem*)(hs + l.items);
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = srcs[(size_t)i];
        DirectRenderItem& it = items[i];
        std::memset(&it, 0, sizeof(it));
        it.state = (DirectRenderState*)s->d_dr;
        it.ring = (float*)(s->d_dr + kDirectRenderHeader);
        it.table = s->dr_table;
        it.mask = s->dr_ring - 1u;
        it.d1 = targets[i].delay * fs_f;
        for (int b = 0; b < B; ++b) it.g1[b] = targets[i].band_gain[b];
    }
    std::memcpy(hs + l.in, in, sizeof(float) * row * (size_t)count);
    FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
    DirectRenderBatch b{};
    b.items = (const DirectRenderItem*)(ds + l.items);
    b.plans = (DirectRenderPlan*)(ds + l.d_plans);
    b.count = count; b.frame = frame; b.taps = srcs[0]->dr_taps; b.bands = B;
    b.in = (const float*)(ds + l.in);
    b.out = (float*)(ds + l.d_out);
    b.mix = mix ? (float*)(ds + l.d_mix) : nullptr;
    launch_direct_render(b, rs);
    FS_HIP(ctx, hipGetLastError());
    if (out)   // out | mix are adjacent on both sides: one copy back
        FS_HIP(ctx, hipMemcpyAsync(hs + l.h_out, ds + l.d_out, sizeof(float) * row * ((size_t)count + (mix ? 1 : 0)), hipMemcpyDeviceToHost, rs));
    else
        FS_HIP(ctx, hipMemcpyAsync(hs + l.h_mix, ds + l.d_mix, sizeof(float) * row, hipMemcpyDeviceToHost, rs));
    FS_HIP(ctx, hipStreamSynchronize(rs));
    if (out) std::memcpy(out, hs + l.h_out, sizeof(float) * row * (size_t)count);
    if (mix) std::memcpy(mix, hs + l.h_mix, sizeof(float) * row);
    return FS_OK;
}

}  // extern "C"
