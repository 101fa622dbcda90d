// fs_capi_paths.cpp — the path queries of a tick, each one call for all its sources: fs_update_direct_paths (fs_direct.hip) with the
// sample offsets it uses, fs_update_reflection_paths (fs_reflect.hip), fs_update_diffraction_paths (fs_diffract.hip),
// fs_update_reflection2_paths (fs_reflect2.hip) and fs_update_diffraction2_paths (fs_diffract2.hip), their defaults, and what the
// five share on the host: the prologue, the staging, the packing of the sources and the copy back.
#include "fs_context.hpp"

static_assert(sizeof(fs_direct_params) == 32, "fs_direct_params: eight words");
static_assert(sizeof(fs_direct_path) == 52, "fs_direct_path: five words and the bands");
static_assert(sizeof(fs_reflection_params) == 36, "fs_reflection_params: nine words");
static_assert(sizeof(fs_reflection_path) == 72, "fs_reflection_path: ten words and the bands");
static_assert(sizeof(fs_reflection_row) == 16, "fs_reflection_row: four words");
static_assert(sizeof(fs_diffraction_params) == 44, "fs_diffraction_params: eleven words");
static_assert(sizeof(fs_diffraction_path) == 84, "fs_diffraction_path: thirteen words and the bands");
static_assert(sizeof(fs_diffraction_row) == 20, "fs_diffraction_row: five words");
static_assert(sizeof(fs_reflection2_params) == 44, "fs_reflection2_params: eleven words");
static_assert(sizeof(fs_reflection2_path) == 92, "fs_reflection2_path: fifteen words and the bands");
static_assert(sizeof(fs_reflection2_row) == 20, "fs_reflection2_row: five words");
static_assert(sizeof(fs_diffraction2_params) == 52, "fs_diffraction2_params: thirteen words");
static_assert(sizeof(fs_diffraction2_path) == 116, "fs_diffraction2_path: twenty-one words and the bands");
static_assert(offsetof(fs_diffraction2_path, detour) == 8 && offsetof(fs_diffraction2_path, gap) == 12 && offsetof(fs_diffraction2_path, cos_bend) == 16 &&
                  offsetof(fs_diffraction2_path, apex) == 24 && offsetof(fs_diffraction2_path, direction) == 48 &&
                  offsetof(fs_diffraction2_path, triangle) == 60 && offsetof(fs_diffraction2_path, edge) == 68 &&
                  offsetof(fs_diffraction2_path, material) == 76 && offsetof(fs_diffraction2_path, gain) == 84,
              "fs_diffraction2_path: the offsets of include/frequensee.h");
static_assert(sizeof(fs_diffraction2_row) == 24, "fs_diffraction2_row: six words");

int PathStaging::grow(fs_context* ctx, int count, size_t pinned_bytes_per_row, size_t device_bytes_per_row) {
    if (count <= cap) return FS_OK;
    // (every earlier call has been waited for: nothing in the stream reads the old staging)
    int rows = std::max(cap, 32);
    while (rows < count) rows *= 2;
    release();
    FS_HIP(ctx, hipHostMalloc((void**)&h, (size_t)rows * pinned_bytes_per_row, hipHostMallocDefault));
    FS_HIP(ctx, hipMalloc((void**)&d, (size_t)rows * device_bytes_per_row));
    cap = rows;
    return FS_OK;
}

void PathStaging::release() {
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    h = nullptr; d = nullptr; cap = 0;
}

namespace {

bool finite_at_least_zero(float x) { return std::isfinite(x) && x >= 0.f; }
bool finite_above_zero(float x) { return std::isfinite(x) && x > 0.f; }

// What every query does between the validation of its own arguments and its first allocation, in this order: the device, the
// handles, the commit, the scene brought up to date.
int paths_prologue(fs_context* ctx, const fs_source* sources, int32_t count) {
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    for (int32_t i = 0; i < count; ++i)
        if (!get_source(ctx, sources[i])) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    { int ir = maybe_install_refined(ctx); if (ir) return ir; }                     // fs_scene_commit_progressive: the better tree is ready
    if (ctx->refit_pending) { int rr = fs_scene_refit(ctx); if (rr) return rr; }   // moved triangles: refit before tracing
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    return FS_OK;
}

// the rows' sources as the kernels read them: xyz + the actor id as bits
void pack_sources(fs_context* ctx, const fs_source* sources, int32_t count, float4* h_src) {
    for (int32_t i = 0; i < count; ++i) {
        const Source* s = get_source(ctx, sources[i]);
        h_src[i] = make_float4(s->pos[0], s->pos[1], s->pos[2], 0.0f);
        std::memcpy(&h_src[i].w, &s->object, sizeof(uint32_t));
    }
}

PathKHead path_head(const fs_context* ctx, const float4* src, int32_t count, float step, float pullback, float dist_divisor, float sound_speed) {
    PathKHead h{};
    h.src = src;
    std::memcpy(h.lis, ctx->listener, sizeof(h.lis));
    h.lis_object = ctx->listener_object;
    h.count = count;
    h.num_bands = ctx->cfg.num_bands;
    h.step = step;
    h.pullback = pullback;
    h.dist_divisor = dist_divisor;
    h.sound_speed = sound_speed;
    return h;
}

// A scan-and-confirm query's device results — rows [count], then paths [count][max_paths] — through the pinned staging into the
// caller's two arrays; waits for the call's kernels.
int copy_back_rows_paths(fs_context* ctx, char* h_out, const char* d_out, size_t rows_bytes, size_t paths_bytes, void* rows, void* paths) {
    FS_HIP(ctx, hipMemcpyAsync(h_out, d_out, rows_bytes + paths_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(rows, h_out, rows_bytes);
    std::memcpy(paths, h_out + rows_bytes, paths_bytes);
    return FS_OK;
}

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

// ctx->diffract_f = the band centres of the edges in force: once per (context, edges in force)
void refresh_band_centres(fs_context* ctx) {
    if (ctx->diffract_f_edges == ctx->band_edges && ctx->diffract_f_bands == ctx->cfg.num_bands) return;
    band_centres(ctx->band_edges, ctx->cfg.num_bands, ctx->diffract_f);
    ctx->diffract_f_edges = ctx->band_edges;
    ctx->diffract_f_bands = ctx->cfg.num_bands;
}

}  // namespace

extern "C" {

// ---- direct paths -----------------------------------------------------------------------------------------------------------
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
        !finite_at_least_zero(p->source_radius) || !finite_at_least_zero(p->step) || !finite_at_least_zero(p->pullback) ||
        !finite_above_zero(p->dist_divisor) || !finite_above_zero(p->sound_speed))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad direct-path params");
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    PathStaging& st = ctx->direct_stage;
    { int gr = st.grow(ctx, count, sizeof(float4) + sizeof(fs_direct_path), sizeof(fs_direct_path)); if (gr) return gr; }
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
    float4* h_src = reinterpret_cast<float4*>(st.h);
    fs_direct_path* h_out = reinterpret_cast<fs_direct_path*>(st.h + (size_t)st.cap * sizeof(float4));
    fs_direct_path* d_out = reinterpret_cast<fs_direct_path*>(st.d);
    pack_sources(ctx, sources, count, h_src);
    DirectKParams dp{};
    dp.h = path_head(ctx, h_src, count, p->step, p->pullback, p->dist_divisor, p->sound_speed);
    dp.offsets = d_off;
    dp.out = d_out;
    dp.samples = n;
    dp.max_surfaces = p->max_surfaces;
    dp.radius = p->source_radius;
    launch_direct_paths(ctx->scene, dp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipMemcpyAsync(h_out, d_out, sizeof(fs_direct_path) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, h_out, sizeof(fs_direct_path) * (size_t)count);
    return FS_OK;
}

// ---- reflection paths -------------------------------------------------------------------------------------------------------
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
        !finite_at_least_zero(p->pullback) || !finite_above_zero(p->dist_divisor) || !finite_above_zero(p->sound_speed))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad reflection-path params");
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    constexpr size_t kCand = FS_MAX_REFLECTION_CANDIDATES;
    constexpr size_t kOutPerRow = sizeof(fs_reflection_row) + FS_MAX_REFLECTIONS * sizeof(fs_reflection_path);
    PathStaging& st = ctx->reflect_stage;
    { int gr = st.grow(ctx, count, sizeof(float4) + kOutPerRow, sizeof(float4) + sizeof(uint32_t) * (1 + kCand) + kOutPerRow); if (gr) return gr; }
    const size_t cap = (size_t)st.cap;
    float4* h_src = reinterpret_cast<float4*>(st.h);
    char* h_out = st.h + cap * sizeof(float4);
    float4* d_src = reinterpret_cast<float4*>(st.d);
    uint32_t* d_counters = reinterpret_cast<uint32_t*>(st.d + cap * sizeof(float4));
    uint32_t* d_cand = d_counters + cap;
    char* d_out = reinterpret_cast<char*>(d_cand + cap * kCand);
    const size_t rows_bytes = sizeof(fs_reflection_row) * (size_t)count;
    pack_sources(ctx, sources, count, h_src);
    ReflectKParams rp{};
    rp.h = path_head(ctx, d_src, count, p->step, p->pullback, p->dist_divisor, p->sound_speed);
    rp.counters = d_counters;
    rp.cand = d_cand;
    rp.rows = reinterpret_cast<fs_reflection_row*>(d_out);
    rp.paths = reinterpret_cast<fs_reflection_path*>(d_out + rows_bytes);
    rp.max_paths = p->max_paths;
    rp.max_candidates = p->max_candidates;
    rp.margin = p->margin;
    rp.offset = p->offset;
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(uint32_t) * (size_t)count, ctx->stream));
    launch_reflection_paths(ctx->scene, rp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    return copy_back_rows_paths(ctx, h_out, d_out, rows_bytes, sizeof(fs_reflection_path) * (size_t)count * (size_t)p->max_paths, rows, paths);
}

// ---- diffraction paths ------------------------------------------------------------------------------------------------------
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
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    constexpr size_t kCand = FS_MAX_DIFFRACTION_CANDIDATES;
    constexpr size_t kOutPerRow = sizeof(fs_diffraction_row) + FS_MAX_DIFFRACTIONS * sizeof(fs_diffraction_path);
    PathStaging& st = ctx->diffract_stage;
    { int gr = st.grow(ctx, count, sizeof(float4) + kOutPerRow,
                       sizeof(float4) + sizeof(DiffractRecord) * kCand + sizeof(uint32_t) * (1 + kCand) + kOutPerRow); if (gr) return gr; }
    refresh_band_centres(ctx);
    const size_t cap = (size_t)st.cap;
    float4* h_src = reinterpret_cast<float4*>(st.h);
    char* h_out = st.h + cap * sizeof(float4);
    float4* d_src = reinterpret_cast<float4*>(st.d);
    DiffractRecord* d_conf = reinterpret_cast<DiffractRecord*>(st.d + cap * sizeof(float4));
    uint32_t* d_counters = reinterpret_cast<uint32_t*>(d_conf + cap * kCand);
    uint32_t* d_cand = d_counters + cap;
    char* d_out = reinterpret_cast<char*>(d_cand + cap * kCand);
    const size_t rows_bytes = sizeof(fs_diffraction_row) * (size_t)count;
    pack_sources(ctx, sources, count, h_src);
    DiffractKParams dp{};
    dp.h = path_head(ctx, d_src, count, p->step, p->pullback, p->dist_divisor, p->sound_speed);
    dp.counters = d_counters;
    dp.cand = d_cand;
    dp.conf = d_conf;
    dp.rows = reinterpret_cast<fs_diffraction_row*>(d_out);
    dp.paths = reinterpret_cast<fs_diffraction_path*>(d_out + rows_bytes);
    dp.max_paths = p->max_paths;
    dp.max_candidates = p->max_candidates;
    dp.margin = p->margin;
    dp.max_detour = p->max_detour;
    dp.offset = p->offset;
    dp.merge = p->merge;
    // k_b travels with the launch's arguments: eight words, no table on the device
    for (int b = 0; b < ctx->cfg.num_bands; ++b) dp.k[b] = (float)(40.0 * ctx->diffract_f[b] / ((double)p->sound_speed * (double)p->dist_divisor));
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(uint32_t) * (size_t)count, ctx->stream));
    launch_diffraction_paths(ctx->scene, dp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    return copy_back_rows_paths(ctx, h_out, d_out, rows_bytes, sizeof(fs_diffraction_path) * (size_t)count * (size_t)p->max_paths, rows, paths);
}

// ---- second-order reflection paths ------------------------------------------------------------------------------------------
void fs_reflection2_params_default(fs_reflection2_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_reflection2_params);
    p->max_paths = 16;
    p->max_near = 16384;
    p->max_candidates = 256;
    p->max_length = 1500.f;   // (2000 leaves most old_mine rows beyond max_near: DESIGN.md "Second-order reflection paths")
    p->margin = 1e-3f;
    p->step = 0.1f;
    p->offset = 0.1f;
    p->pullback = 0.1f;
    p->dist_divisor = 1000.f;
    p->sound_speed = 343.f;
}

int fs_update_reflection2_paths(fs_context* ctx, const fs_source* sources, int32_t count, const fs_reflection2_params* p,
                                fs_reflection2_row* rows, fs_reflection2_path* paths) {
    if (!ctx || !sources || !rows || !paths) return FS_ERR_INVALID_ARGUMENT;
    if (count < 1 || count > FS_MAX_REFLECTION2_BATCH) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REFLECTION2_BATCH)");
    fs_reflection2_params def;
    if (!p) { fs_reflection2_params_default(&def); p = &def; }
    if (p->struct_size != sizeof(fs_reflection2_params)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reflection2_params.struct_size mismatch");
    if (p->max_paths < 1 || p->max_paths > FS_MAX_REFLECTION2_PATHS || p->max_near < 1 || p->max_near > FS_MAX_REFLECTION2_NEAR ||
        p->max_candidates < 1 || p->max_candidates > FS_MAX_REFLECTION2_CANDIDATES || !finite_above_zero(p->max_length) ||
        !finite_at_least_zero(p->margin) || !finite_at_least_zero(p->step) || !finite_at_least_zero(p->offset) ||
        !finite_at_least_zero(p->pullback) || !finite_above_zero(p->dist_divisor) || !finite_above_zero(p->sound_speed))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad second-order reflection-path params");
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    constexpr size_t kNear = FS_MAX_REFLECTION2_NEAR, kCand = FS_MAX_REFLECTION2_CANDIDATES;
    constexpr size_t kOutPerRow = sizeof(fs_reflection2_row) + FS_MAX_REFLECTION2_PATHS * sizeof(fs_reflection2_path);
    PathStaging& st = ctx->reflect2_stage;
    { int gr = st.grow(ctx, count, sizeof(float4) + kOutPerRow,
                       sizeof(float4) + sizeof(uint32_t) * (2 + kNear + kCand) + sizeof(Reflect2Record) * kCand + kOutPerRow); if (gr) return gr; }
    const size_t cap = (size_t)st.cap;
    float4* h_src = reinterpret_cast<float4*>(st.h);
    char* h_out = st.h + cap * sizeof(float4);
    float4* d_src = reinterpret_cast<float4*>(st.d);
    uint32_t* d_near_counters = reinterpret_cast<uint32_t*>(st.d + cap * sizeof(float4));
    uint32_t* d_counters = d_near_counters + cap;
    uint32_t* d_near = d_counters + cap;
    uint32_t* d_cand = d_near + cap * kNear;
    Reflect2Record* d_conf = reinterpret_cast<Reflect2Record*>(d_cand + cap * kCand);
    char* d_out = reinterpret_cast<char*>(d_conf + cap * kCand);
    const size_t rows_bytes = sizeof(fs_reflection2_row) * (size_t)count;
    pack_sources(ctx, sources, count, h_src);
    Reflect2KParams rp{};
    rp.h = path_head(ctx, d_src, count, p->step, p->pullback, p->dist_divisor, p->sound_speed);
    rp.near_counters = d_near_counters;
    rp.counters = d_counters;
    rp.near = d_near;
    rp.cand = d_cand;
    rp.conf = d_conf;
    rp.rows = reinterpret_cast<fs_reflection2_row*>(d_out);
    rp.paths = reinterpret_cast<fs_reflection2_path*>(d_out + rows_bytes);
    rp.max_paths = p->max_paths;
    rp.max_near = p->max_near;
    rp.max_candidates = p->max_candidates;
    rp.max_length = p->max_length;
    rp.margin = p->margin;
    rp.offset = p->offset;
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemsetAsync(d_near_counters, 0, sizeof(uint32_t) * 2 * cap, ctx->stream));   // both counter arrays: they lie side by side
    launch_reflection2_paths(ctx->scene, rp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    return copy_back_rows_paths(ctx, h_out, d_out, rows_bytes, sizeof(fs_reflection2_path) * (size_t)count * (size_t)p->max_paths, rows, paths);
}

// ---- second-order diffraction paths -----------------------------------------------------------------------------------------
void fs_diffraction2_params_default(fs_diffraction2_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_diffraction2_params);
    p->max_paths = 4;
    p->max_near = 16384;
    p->max_candidates = 1024;
    p->margin = 1e-3f;
    p->max_detour = 250.f;    // (at the first-order call's 1000 every old_mine row overflows max_near: DESIGN.md "Second-order diffraction paths")
    p->min_parallel = 0.999f;
    p->offset = 0.1f;
    p->merge = 1.0f;
    p->step = 0.1f;
    p->pullback = 0.1f;
    p->dist_divisor = 1000.f;
    p->sound_speed = 343.f;
}

int fs_update_diffraction2_paths(fs_context* ctx, const fs_source* sources, int32_t count, const fs_diffraction2_params* p,
                                 fs_diffraction2_row* rows, fs_diffraction2_path* paths) {
    if (!ctx || !sources || !rows || !paths) return FS_ERR_INVALID_ARGUMENT;
    if (count < 1 || count > FS_MAX_DIFFRACTION2_BATCH) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_DIFFRACTION2_BATCH)");
    fs_diffraction2_params def;
    if (!p) { fs_diffraction2_params_default(&def); p = &def; }
    if (p->struct_size != sizeof(fs_diffraction2_params)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_diffraction2_params.struct_size mismatch");
    if (p->max_paths < 1 || p->max_paths > FS_MAX_DIFFRACTION2_PATHS || p->max_near < 1 || p->max_near > FS_MAX_DIFFRACTION2_NEAR ||
        p->max_candidates < 1 || p->max_candidates > FS_MAX_DIFFRACTION2_CANDIDATES || !finite_at_least_zero(p->margin) ||
        !finite_above_zero(p->max_detour) || !finite_above_zero(p->min_parallel) || p->min_parallel > 1.0f || !finite_at_least_zero(p->offset) ||
        !finite_at_least_zero(p->merge) || !finite_at_least_zero(p->step) || !finite_at_least_zero(p->pullback) ||
        !finite_above_zero(p->dist_divisor) || !finite_above_zero(p->sound_speed))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad second-order diffraction-path params");
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    constexpr size_t kNear = FS_MAX_DIFFRACTION2_NEAR, kCand = FS_MAX_DIFFRACTION2_CANDIDATES;
    constexpr size_t kOutPerRow = sizeof(fs_diffraction2_row) + FS_MAX_DIFFRACTION2_PATHS * sizeof(fs_diffraction2_path);
    PathStaging& st = ctx->diffract2_stage;
    { int gr = st.grow(ctx, count, sizeof(float4) + kOutPerRow,
                       sizeof(float4) + sizeof(uint32_t) * (2 + kNear + kCand) + sizeof(Diffract2Record) * kCand + kOutPerRow); if (gr) return gr; }
    refresh_band_centres(ctx);
    const size_t cap = (size_t)st.cap;
    float4* h_src = reinterpret_cast<float4*>(st.h);
    char* h_out = st.h + cap * sizeof(float4);
    float4* d_src = reinterpret_cast<float4*>(st.d);
    uint32_t* d_near_counters = reinterpret_cast<uint32_t*>(st.d + cap * sizeof(float4));
    uint32_t* d_counters = d_near_counters + cap;
    uint32_t* d_near = d_counters + cap;
    uint32_t* d_cand = d_near + cap * kNear;
    Diffract2Record* d_conf = reinterpret_cast<Diffract2Record*>(d_cand + cap * kCand);
    char* d_out = reinterpret_cast<char*>(d_conf + cap * kCand);
    const size_t rows_bytes = sizeof(fs_diffraction2_row) * (size_t)count;
    pack_sources(ctx, sources, count, h_src);
    Diffract2KParams dp{};
    dp.h = path_head(ctx, d_src, count, p->step, p->pullback, p->dist_divisor, p->sound_speed);
    dp.near_counters = d_near_counters;
    dp.counters = d_counters;
    dp.near = d_near;
    dp.cand = d_cand;
    dp.conf = d_conf;
    dp.rows = reinterpret_cast<fs_diffraction2_row*>(d_out);
    dp.paths = reinterpret_cast<fs_diffraction2_path*>(d_out + rows_bytes);
    dp.max_paths = p->max_paths;
    dp.max_near = p->max_near;
    dp.max_candidates = p->max_candidates;
    dp.margin = p->margin;
    dp.max_detour = p->max_detour;
    dp.min_parallel = p->min_parallel;
    dp.offset = p->offset;
    dp.merge = p->merge;
    // k_b and lam5_b travel with the launch's arguments: sixteen words, no table on the device
    for (int b = 0; b < ctx->cfg.num_bands; ++b) {
        dp.k[b] = (float)(40.0 * ctx->diffract_f[b] / ((double)p->sound_speed * (double)p->dist_divisor));
        dp.lam5[b] = (float)(5.0 * (double)p->sound_speed * (double)p->dist_divisor / ctx->diffract_f[b]);
    }
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemsetAsync(d_near_counters, 0, sizeof(uint32_t) * 2 * cap, ctx->stream));   // both counter arrays: they lie side by side
    launch_diffraction2_paths(ctx->scene, dp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    return copy_back_rows_paths(ctx, h_out, d_out, rows_bytes, sizeof(fs_diffraction2_path) * (size_t)count * (size_t)p->max_paths, rows, paths);
}

}  // extern "C"
