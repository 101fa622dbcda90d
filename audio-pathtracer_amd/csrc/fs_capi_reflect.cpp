// fs_capi_reflect.cpp — reflection paths: fs_update_reflection_paths (the scan and the confirmation of all sources of a tick,
// fs_reflect.hip) and its defaults.
#include "fs_context.hpp"

static_assert(sizeof(fs_reflection_params) == 36, "fs_reflection_params: nine words");
static_assert(sizeof(fs_reflection_path) == 72, "fs_reflection_path: ten words and the bands");
static_assert(sizeof(fs_reflection_row) == 16, "fs_reflection_row: four words");

namespace {
// bytes of a call's rows [count] followed by its paths [count][max_paths]: what the copy back moves
constexpr size_t reflect_out_bytes(size_t count, size_t max_paths) {
    return count * (sizeof(fs_reflection_row) + max_paths * sizeof(fs_reflection_path));
}
bool finite_at_least_zero(float x) { return std::isfinite(x) && x >= 0.f; }
}  // namespace

extern "C" {

void fs_reflection_params_default(fs_reflection_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_reflection_params);
    p->max_paths = 8;
    p->max_candidates = FS_MAX_REFLECTION_CANDIDATES;
    p->margin = 1e-3f;
    p->step = 0.1f;
    p->offset = 0.1f;
    p->pullback = 0.1f;
    p->dist_divisor = 1000.f;
    p->sound_speed = 343.f;
}

int fs_update_reflection_paths(fs_context* ctx, const fs_source* sources, int32_t count, const fs_reflection_params* p,
                               fs_reflection_row* rows, fs_reflection_path* paths) {
    if (!ctx || !sources || !rows || !paths) return FS_ERR_INVALID_ARGUMENT;
    if (count < 1 || count > FS_MAX_REFLECTION_BATCH) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REFLECTION_BATCH)");
    fs_reflection_params def;
    if (!p) { fs_reflection_params_default(&def); p = &def; }
    if (p->struct_size != sizeof(fs_reflection_params)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reflection_params.struct_size mismatch");
    if (p->max_paths < 1 || p->max_paths > FS_MAX_REFLECTIONS || p->max_candidates < 1 || p->max_candidates > FS_MAX_REFLECTION_CANDIDATES ||
        !finite_at_least_zero(p->margin) || !finite_at_least_zero(p->step) || !finite_at_least_zero(p->offset) ||
        !finite_at_least_zero(p->pullback) || !std::isfinite(p->dist_divisor) || !(p->dist_divisor > 0.f) ||
        !std::isfinite(p->sound_speed) || !(p->sound_speed > 0.f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad reflection-path params");
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    for (int32_t i = 0; i < count; ++i)
        if (!get_source(ctx, sources[i])) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    { int ir = maybe_install_refined(ctx); if (ir) return ir; }                     // fs_scene_commit_progressive: the better tree is ready
    if (ctx->refit_pending) { int rr = fs_scene_refit(ctx); if (rr) return rr; }   // moved triangles: refit before tracing
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    constexpr size_t kCand = FS_MAX_REFLECTION_CANDIDATES;
    if (count > ctx->reflect_cap) {   // (every earlier call has been waited for: nothing in the stream reads the old staging)
        int cap = std::max(ctx->reflect_cap, 32);
        while (cap < count) cap *= 2;
        if (ctx->h_reflect) (void)hipHostFree(ctx->h_reflect);
        if (ctx->d_reflect) (void)hipFree(ctx->d_reflect);
        ctx->h_reflect = nullptr; ctx->d_reflect = nullptr; ctx->reflect_cap = 0;
        const size_t out_bytes = reflect_out_bytes((size_t)cap, FS_MAX_REFLECTIONS);
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_reflect, (size_t)cap * sizeof(float4) + out_bytes, hipHostMallocDefault));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_reflect, (size_t)cap * (sizeof(float4) + sizeof(uint32_t) * (1 + kCand)) + out_bytes));
        ctx->reflect_cap = cap;
    }
    const size_t cap = (size_t)ctx->reflect_cap;
    float4* h_src = reinterpret_cast<float4*>(ctx->h_reflect);
    char* h_out = ctx->h_reflect + cap * sizeof(float4);
    float4* d_src = reinterpret_cast<float4*>(ctx->d_reflect);
    uint32_t* d_counters = reinterpret_cast<uint32_t*>(ctx->d_reflect + cap * sizeof(float4));
    uint32_t* d_cand = d_counters + cap;
    char* d_out = reinterpret_cast<char*>(d_cand + cap * kCand);
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = get_source(ctx, sources[i]);
        h_src[i] = make_float4(s->pos[0], s->pos[1], s->pos[2], 0.0f);
        std::memcpy(&h_src[i].w, &s->object, sizeof(uint32_t));   // the actor id as bits
    }
    ReflectKParams rp{};
    rp.src = d_src;
    rp.counters = d_counters;
    rp.cand = d_cand;
    rp.rows = reinterpret_cast<fs_reflection_row*>(d_out);
    rp.paths = reinterpret_cast<fs_reflection_path*>(d_out + (size_t)count * sizeof(fs_reflection_row));
    std::memcpy(rp.lis, ctx->listener, sizeof(rp.lis));
    rp.lis_object = ctx->listener_object;
    rp.count = count;
    rp.max_paths = p->max_paths;
    rp.max_candidates = p->max_candidates;
    rp.num_bands = ctx->cfg.num_bands;
    rp.margin = p->margin;
    rp.step = p->step;
    rp.offset = p->offset;
    rp.pullback = p->pullback;
    rp.dist_divisor = p->dist_divisor;
    rp.sound_speed = p->sound_speed;
    const size_t out_bytes = reflect_out_bytes((size_t)count, (size_t)p->max_paths);
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(uint32_t) * (size_t)count, ctx->stream));
    launch_reflection_paths(ctx->scene, rp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(rows, h_out, sizeof(fs_reflection_row) * (size_t)count);
    std::memcpy(paths, h_out + (size_t)count * sizeof(fs_reflection_row), sizeof(fs_reflection_path) * (size_t)count * (size_t)p->max_paths);
    return FS_OK;
}

}  // extern "C"
