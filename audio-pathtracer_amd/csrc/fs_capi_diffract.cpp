// fs_capi_diffract.cpp — diffraction paths: fs_update_diffraction_paths (the scan and the confirmation of all sources of a tick,
// fs_diffract.hip) and its defaults.
#include "fs_context.hpp"

static_assert(sizeof(fs_diffraction_params) == 44, "fs_diffraction_params: eleven words");
static_assert(sizeof(fs_diffraction_path) == 84, "fs_diffraction_path: thirteen words and the bands");
static_assert(sizeof(fs_diffraction_row) == 20, "fs_diffraction_row: five words");

namespace {
// bytes of a call's rows [count] followed by its paths [count][max_paths]: what the copy back moves
constexpr size_t diffract_out_bytes(size_t count, size_t max_paths) {
    return count * (sizeof(fs_diffraction_row) + max_paths * sizeof(fs_diffraction_path));
}
bool finite_at_least_zero(float x) { return std::isfinite(x) && x >= 0.f; }
bool finite_above_zero(float x) { return std::isfinite(x) && x > 0.f; }

// f_b of the header: the geometric mean of each band's edges, the outer bands with an octave-wide virtual edge
void band_centres(const std::vector<double>& given, int B, double* f) {
    std::vector<double> e = given;
    if (e.empty())
        for (int b = 1; b < B; ++b) e.push_back(125.0 * std::pow(2.0, (double)b - 0.5));   // the default octave edges
    if (B == 1) { f[0] = 1000.0; return; }
    for (int b = 0; b < B; ++b) {
        const double lo = b == 0 ? e[0] / 2.0 : e[(size_t)b - 1], hi = b == B - 1 ? e[(size_t)B - 2] * 2.0 : e[(size_t)b];
        f[b] = std::sqrt(lo * hi);
    }
}
}  // namespace

extern "C" {

void fs_diffraction_params_default(fs_diffraction_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_diffraction_params);
    p->max_paths = 4;
    p->max_candidates = 1024;
    p->margin = 1e-3f;
    p->max_detour = 1000.f;
    p->offset = 0.1f;
    p->merge = 1.0f;
    p->step = 0.1f;
    p->pullback = 0.1f;
    p->dist_divisor = 1000.f;
    p->sound_speed = 343.f;
}

int fs_update_diffraction_paths(fs_context* ctx, const fs_source* sources, int32_t count, const fs_diffraction_params* p,
                                fs_diffraction_row* rows, fs_diffraction_path* paths) {
    if (!ctx || !sources || !rows || !paths) return FS_ERR_INVALID_ARGUMENT;
    if (count < 1 || count > FS_MAX_DIFFRACTION_BATCH) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_DIFFRACTION_BATCH)");
    fs_diffraction_params def;
    if (!p) { fs_diffraction_params_default(&def); p = &def; }
    if (p->struct_size != sizeof(fs_diffraction_params)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_diffraction_params.struct_size mismatch");
    if (p->max_paths < 1 || p->max_paths > FS_MAX_DIFFRACTIONS || p->max_candidates < 1 || p->max_candidates > FS_MAX_DIFFRACTION_CANDIDATES ||
        !finite_at_least_zero(p->margin) || !finite_above_zero(p->max_detour) || !finite_at_least_zero(p->offset) ||
        !finite_at_least_zero(p->merge) || !finite_at_least_zero(p->step) || !finite_at_least_zero(p->pullback) ||
        !finite_above_zero(p->dist_divisor) || !finite_above_zero(p->sound_speed))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad diffraction-path params");
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    for (int32_t i = 0; i < count; ++i)
        if (!get_source(ctx, sources[i])) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    { int ir = maybe_install_refined(ctx); if (ir) return ir; }                     // fs_scene_commit_progressive: the better tree is ready
    if (ctx->refit_pending) { int rr = fs_scene_refit(ctx); if (rr) return rr; }   // moved triangles: refit before tracing
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    constexpr size_t kCand = FS_MAX_DIFFRACTION_CANDIDATES;
    if (count > ctx->diffract_cap) {   // (every earlier call has been waited for: nothing in the stream reads the old staging)
        int cap = std::max(ctx->diffract_cap, 32);
        while (cap < count) cap *= 2;
        if (ctx->h_diffract) (void)hipHostFree(ctx->h_diffract);
        if (ctx->d_diffract) (void)hipFree(ctx->d_diffract);
        ctx->h_diffract = nullptr; ctx->d_diffract = nullptr; ctx->diffract_cap = 0;
        const size_t out_bytes = diffract_out_bytes((size_t)cap, FS_MAX_DIFFRACTIONS);
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_diffract, (size_t)cap * sizeof(float4) + out_bytes, hipHostMallocDefault));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_diffract,
                              (size_t)cap * (sizeof(float4) + sizeof(fs::DiffractRecord) * kCand + sizeof(uint32_t) * (1 + kCand)) + out_bytes));
        ctx->diffract_cap = cap;
    }
    if (ctx->diffract_f_edges != ctx->band_edges || ctx->diffract_f_bands != ctx->cfg.num_bands) {   // once per (context, edges in force)
        band_centres(ctx->band_edges, ctx->cfg.num_bands, ctx->diffract_f);
        ctx->diffract_f_edges = ctx->band_edges;
        ctx->diffract_f_bands = ctx->cfg.num_bands;
    }
    const size_t cap = (size_t)ctx->diffract_cap;
    float4* h_src = reinterpret_cast<float4*>(ctx->h_diffract);
    char* h_out = ctx->h_diffract + cap * sizeof(float4);
    float4* d_src = reinterpret_cast<float4*>(ctx->d_diffract);
    fs::DiffractRecord* d_conf = reinterpret_cast<fs::DiffractRecord*>(ctx->d_diffract + cap * sizeof(float4));
    uint32_t* d_counters = reinterpret_cast<uint32_t*>(d_conf + cap * kCand);
    uint32_t* d_cand = d_counters + cap;
    char* d_out = reinterpret_cast<char*>(d_cand + cap * kCand);
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = get_source(ctx, sources[i]);
        h_src[i] = make_float4(s->pos[0], s->pos[1], s->pos[2], 0.0f);
        std::memcpy(&h_src[i].w, &s->object, sizeof(uint32_t));   // the actor id as bits
    }
    fs::DiffractKParams dp{};
    dp.src = d_src;
    dp.counters = d_counters;
    dp.cand = d_cand;
    dp.conf = d_conf;
    dp.rows = reinterpret_cast<fs_diffraction_row*>(d_out);
    dp.paths = reinterpret_cast<fs_diffraction_path*>(d_out + (size_t)count * sizeof(fs_diffraction_row));
    std::memcpy(dp.lis, ctx->listener, sizeof(dp.lis));
    dp.lis_object = ctx->listener_object;
    dp.count = count;
    dp.max_paths = p->max_paths;
    dp.max_candidates = p->max_candidates;
    dp.num_bands = ctx->cfg.num_bands;
    dp.margin = p->margin;
    dp.max_detour = p->max_detour;
    dp.offset = p->offset;
    dp.merge = p->merge;
    dp.step = p->step;
    dp.pullback = p->pullback;
    dp.dist_divisor = p->dist_divisor;
    dp.sound_speed = p->sound_speed;
    // k_b travels with the launch's arguments: eight words, no table on the device
    for (int b = 0; b < ctx->cfg.num_bands; ++b) dp.k[b] = (float)(40.0 * ctx->diffract_f[b] / ((double)p->sound_speed * (double)p->dist_divisor));
    const size_t out_bytes = diffract_out_bytes((size_t)count, (size_t)p->max_paths);
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(uint32_t) * (size_t)count, ctx->stream));
    fs::launch_diffraction_paths(ctx->scene, dp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(rows, h_out, sizeof(fs_diffraction_row) * (size_t)count);
    std::memcpy(paths, h_out + (size_t)count * sizeof(fs_diffraction_row), sizeof(fs_diffraction_path) * (size_t)count * (size_t)p->max_paths);
    return FS_OK;
}

}  // extern "C"
