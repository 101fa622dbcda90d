// fs_capi_direct.cpp — direct paths: fs_update_direct_paths (one launch for all sources of a tick, fs_direct.hip), the sample
// offsets it uses and its defaults.
#include "fs_context.hpp"

static_assert(sizeof(fs_direct_params) == 32, "fs_direct_params: eight words");
static_assert(sizeof(fs_direct_path) == 52, "fs_direct_path: five words and the bands");

extern "C" {

void fs_direct_params_default(fs_direct_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_direct_params);
    p->samples = 16;
    p->source_radius = 0.0f;
    p->max_surfaces = 8;
    p->step = 0.1f;           // FSAC.cpp:232
    p->pullback = 0.1f;       // ARTS.cpp:253
    p->dist_divisor = 1000.f; // ARTS.cpp:373
    p->sound_speed = 343.f;
}

// the centre, then n - 1 points of a Fibonacci spiral on the unit sphere: in double, rounded to float once
int fs_direct_sample_offsets(int32_t n, float* out) {
    if (n < 1 || n > FS_MAX_DIRECT_SAMPLES || !out) return FS_ERR_INVALID_ARGUMENT;
    out[0] = out[1] = out[2] = 0.0f;
    const double pi = 3.14159265358979323846, m = (double)(n - 1);
    for (int k = 1; k < n; ++k) {
        const double j = (double)(k - 1);
        const double z = 1.0 - (2.0 * j + 1.0) / m;
        const double rho = std::sqrt(1.0 - z * z);
        const double phi = j * pi * (3.0 - std::sqrt(5.0));
        out[3 * k] = (float)(rho * std::cos(phi));
        out[3 * k + 1] = (float)(rho * std::sin(phi));
        out[3 * k + 2] = (float)z;
    }
    return FS_OK;
}

int fs_update_direct_paths(fs_context* ctx, const fs_source* sources, int32_t count, const fs_direct_params* p, fs_direct_path* out) {
    if (!ctx || !sources || !out) return FS_ERR_INVALID_ARGUMENT;
    if (count < 1 || count > FS_MAX_DIRECT_BATCH) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_DIRECT_BATCH)");
    fs_direct_params def;
    if (!p) { fs_direct_params_default(&def); p = &def; }
    if (p->struct_size != sizeof(fs_direct_params)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_direct_params.struct_size mismatch");
    if (p->samples < 1 || p->samples > FS_MAX_DIRECT_SAMPLES || p->max_surfaces < 1 || p->max_surfaces > FS_DIRECT_MAX_QUERIES - 1 ||
        !std::isfinite(p->source_radius) || !(p->source_radius >= 0.f) || !std::isfinite(p->step) || !(p->step >= 0.f) ||
        !std::isfinite(p->pullback) || !(p->pullback >= 0.f) || !std::isfinite(p->dist_divisor) || !(p->dist_divisor > 0.f) ||
        !std::isfinite(p->sound_speed) || !(p->sound_speed > 0.f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad direct-path params");
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    for (int32_t i = 0; i < count; ++i)
        if (!get_source(ctx, sources[i])) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    { int ir = maybe_install_refined(ctx); if (ir) return ir; }                     // fs_scene_commit_progressive: the better tree is ready
    if (ctx->refit_pending) { int rr = fs_scene_refit(ctx); if (rr) return rr; }   // moved triangles: refit before tracing
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (count > ctx->direct_cap) {   // (every earlier call has been waited for: nothing in the stream reads the old staging)
        int cap = std::max(ctx->direct_cap, 32);
        while (cap < count) cap *= 2;
        if (ctx->h_direct) (void)hipHostFree(ctx->h_direct);
        if (ctx->d_direct) (void)hipFree(ctx->d_direct);
        ctx->h_direct = nullptr; ctx->d_direct = nullptr; ctx->direct_cap = 0;
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_direct, (size_t)cap * (sizeof(float4) + sizeof(fs_direct_path)), hipHostMallocDefault));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_direct, (size_t)cap * sizeof(fs_direct_path)));
        ctx->direct_cap = cap;
    }
    const int n = p->source_radius == 0.0f ? 1 : p->samples;
    constexpr size_t kTable = (size_t)FS_MAX_DIRECT_SAMPLES * 3;
    if (!ctx->d_direct_off) FS_HIP(ctx, hipMalloc((void**)&ctx->d_direct_off, sizeof(float) * kTable * FS_MAX_DIRECT_SAMPLES));
    float* d_off = ctx->d_direct_off + kTable * (size_t)(n - 1);
    if (((ctx->direct_off_have >> (n - 1)) & 1ull) == 0ull) {
        float tab[kTable];
        (void)fs_direct_sample_offsets(n, tab);
        FS_HIP(ctx, hipMemcpy(d_off, tab, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice));
        ctx->direct_off_have |= 1ull << (n - 1);
    }
    float4* h_src = reinterpret_cast<float4*>(ctx->h_direct);
    fs_direct_path* h_out = reinterpret_cast<fs_direct_path*>(ctx->h_direct + (size_t)ctx->direct_cap * sizeof(float4));
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = get_source(ctx, sources[i]);
        h_src[i] = make_float4(s->pos[0], s->pos[1], s->pos[2], 0.0f);
        std::memcpy(&h_src[i].w, &s->object, sizeof(uint32_t));   // the actor id as bits
    }
    DirectKParams dp{};
    dp.src = h_src;
    dp.offsets = d_off;
    dp.out = ctx->d_direct;
    std::memcpy(dp.lis, ctx->listener, sizeof(dp.lis));
    dp.lis_object = ctx->listener_object;
    dp.count = count;
    dp.samples = n;
    dp.max_surfaces = p->max_surfaces;
    dp.num_bands = ctx->cfg.num_bands;
    dp.radius = p->source_radius;
    dp.step = p->step;
    dp.pullback = p->pullback;
    dp.dist_divisor = p->dist_divisor;
    dp.sound_speed = p->sound_speed;
    launch_direct_paths(ctx->scene, dp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipMemcpyAsync(h_out, ctx->d_direct, sizeof(fs_direct_path) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, h_out, sizeof(fs_direct_path) * (size_t)count);
    return FS_OK;
}

}  // extern "C"
