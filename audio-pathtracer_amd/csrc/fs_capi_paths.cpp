// fs_capi_paths.cpp — the path queries of a tick, each one call for all its sources: fs_update_direct_paths (fs_direct.hip) with the
// sample offsets it uses, fs_update_reflection_paths (fs_reflect.hip), fs_update_diffraction_paths (fs_diffract.hip),
// fs_update_reflection2_paths (fs_reflect2.hip), fs_update_diffraction2_paths (fs_diffract2.hip) and fs_update_mixed_paths
// (fs_mixed.hip), their defaults, the probe graph's calls (fs_pathing_*, fs_update_pathing_paths: fs_pathing.hip), and what the
// queries share on the host: the prologue, the staging and its layout, the packing of the sources and, for the five that return rows
// and paths, one driver from the argument checks to the copy back (update_rows_paths).
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
static_assert(sizeof(fs_mixed_params) == 52, "fs_mixed_params: thirteen words");
static_assert(sizeof(fs_mixed_path) == 112, "fs_mixed_path: twenty words and the bands");
static_assert(offsetof(fs_mixed_path, detour) == 8 && offsetof(fs_mixed_path, bend_detour) == 12 && offsetof(fs_mixed_path, cos_bend) == 16 &&
                  offsetof(fs_mixed_path, apex) == 20 && offsetof(fs_mixed_path, point) == 32 && offsetof(fs_mixed_path, direction) == 44 &&
                  offsetof(fs_mixed_path, end) == 56 && offsetof(fs_mixed_path, triangle) == 60 && offsetof(fs_mixed_path, edge) == 68 &&
                  offsetof(fs_mixed_path, material) == 72 && offsetof(fs_mixed_path, gain) == 80,
              "fs_mixed_path: the offsets of include/frequensee.h");
static_assert(sizeof(fs_mixed_row) == 24, "fs_mixed_row: six words");
static_assert(sizeof(fs_pathing_bake_params) == 12 && sizeof(fs_pathing_params) == 32, "the pathing params: three and eight words");
static_assert(sizeof(fs_pathing_path) == 152 && offsetof(fs_pathing_path, distance) == 12 && offsetof(fs_pathing_path, direction) == 16 &&
                  offsetof(fs_pathing_path, departure) == 28 && offsetof(fs_pathing_path, hops) == 40 && offsetof(fs_pathing_path, flags) == 44 &&
                  offsetof(fs_pathing_path, probes) == 56 && offsetof(fs_pathing_path, gain) == 120,
              "fs_pathing_path: the offsets of include/frequensee.h");

int PathStaging::grow(fs_context* ctx, int count, const PathLayout& pinned_layout, const PathLayout& device_layout) {
    pinned = pinned_layout;
    device = device_layout;
    if (count <= cap) return FS_OK;
    // (every earlier call has been waited for: nothing in the stream reads the old staging)
    int rows = std::max(cap, 32);
    while (rows < count) rows *= 2;
    release();
    FS_HIP(ctx, hipHostMalloc((void**)&h, (size_t)rows * pinned.before(kPathSegments), hipHostMallocDefault));
    FS_HIP(ctx, hipMalloc((void**)&d, (size_t)rows * device.before(kPathSegments)));
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

// k_b = 40 f_b / (sound_speed dist_divisor) and, where asked for, lam5_b = 5 sound_speed dist_divisor / f_b of the bands in force:
// they travel with the launch's arguments, no table on the device
void band_factors(fs_context* ctx, float sound_speed, float dist_divisor, float* k, float* lam5) {
    refresh_band_centres(ctx);
    for (int b = 0; b < ctx->cfg.num_bands; ++b) {
        k[b] = (float)(40.0 * ctx->diffract_f[b] / ((double)sound_speed * (double)dist_divisor));
        if (lam5) lam5[b] = (float)(5.0 * (double)sound_speed * (double)dist_divisor / ctx->diffract_f[b]);
    }
}

// p, or the query's defaults where the caller passed none; false = a struct_size that is not this library's
template <typename Params>
bool params_or_default(const Params*& p, Params& def, void (*defaults)(Params*)) {
    if (!p) { defaults(&def); p = &def; }
    return p->struct_size == sizeof(Params);
}

// What one of the five rows-and-paths queries is, beyond its kernels: its messages, its staging and the sizes the staging is laid
// out for (per row: counter arrays, near-list and candidate entries, bytes of a confirmed record, paths).
template <typename Params, typename KP>
struct RowsPathsQuery {
    int32_t max_batch;
    const char *bad_count, *bad_size, *bad_params;
    void (*defaults)(Params*);
    PathStaging fs_context::*stage;
    size_t counter_arrays, max_near, max_candidates, record_bytes, max_paths;
    void (*launch)(const DeviceScene&, const KP&, hipStream_t);
};

// A rows-and-paths query from its arguments to the caller's two arrays, every check in the order the header gives.  valid(p) is the
// query's own test of its params; fill(kp, p, st) sets what the kernels read beyond h, rows and paths: the lists of st and the params.
template <typename Params, typename KP, typename Row, typename Path, typename Valid, typename Fill>
int update_rows_paths(const RowsPathsQuery<Params, KP>& q, fs_context* ctx, const fs_source* sources, int32_t count, const Params* p, Row* rows,
                      Path* paths, Valid&& valid, Fill&& fill) {
    if (!ctx || !sources || !rows || !paths) return FS_ERR_INVALID_ARGUMENT;
    if (count < 1 || count > q.max_batch) return ctx->fail(FS_ERR_INVALID_ARGUMENT, q.bad_count);
    Params def;
    if (!params_or_default(p, def, q.defaults)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, q.bad_size);
    if (!valid(*p)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, q.bad_params);
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    const size_t out_per_row = sizeof(Row) + q.max_paths * sizeof(Path);
    PathStaging& st = ctx->*q.stage;
    { int gr = st.grow(ctx, count, PathLayout{{sizeof(float4), 0, 0, 0, 0, out_per_row}},
                       PathLayout{{sizeof(float4), sizeof(uint32_t) * q.counter_arrays, sizeof(uint32_t) * q.max_near, sizeof(uint32_t) * q.max_candidates,
                                   q.record_bytes * q.max_candidates, out_per_row}}); if (gr) return gr; }
    float4* h_src = reinterpret_cast<float4*>(st.host(kSegSources));
    float4* d_src = reinterpret_cast<float4*>(st.dev(kSegSources));
    char *h_out = st.host(kSegOut), *d_out = st.dev(kSegOut);
    const size_t rows_bytes = sizeof(Row) * (size_t)count, paths_bytes = sizeof(Path) * (size_t)count * (size_t)p->max_paths;
    pack_sources(ctx, sources, count, h_src);
    KP kp{};
    kp.h = path_head(ctx, d_src, count, p->step, p->pullback, p->dist_divisor, p->sound_speed);
    kp.rows = reinterpret_cast<Row*>(d_out);
    kp.paths = reinterpret_cast<Path*>(d_out + rows_bytes);
    kp.max_paths = p->max_paths;
    fill(kp, *p, st);
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemsetAsync(st.dev(kSegCounters), 0, st.dev_bytes(kSegCounters), ctx->stream));   // every counter array of the call: one clear
    q.launch(ctx->scene, kp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipMemcpyAsync(h_out, d_out, rows_bytes + paths_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));   // waits for the call's kernels
    std::memcpy(rows, h_out, rows_bytes);
    std::memcpy(paths, h_out + rows_bytes, paths_bytes);
    return FS_OK;
}

// the lists of a first-order query's staging, and of a second-order one's
uint32_t* staged_words(const PathStaging& st, int seg) { return reinterpret_cast<uint32_t*>(st.dev(seg)); }
NearPairLists staged_pair_lists(const PathStaging& st, int32_t max_near, int32_t max_candidates) {
    return NearPairLists{staged_words(st, kSegCounters), staged_words(st, kSegCounters) + st.cap, staged_words(st, kSegNear), staged_words(st, kSegCand),
                         max_near, max_candidates};
}

// the probe set's device block (fs_context::Pathing), laid out for FS_MAX_PATHING_PROBES: probes | upper | graph | dL | d | pred
constexpr size_t kPathingMatrixBytes = sizeof(uint32_t) * (size_t)FS_MAX_PATHING_PROBES * (size_t)kPathingStrideWords;
constexpr size_t kPathingBlockBytes = sizeof(float4) * (size_t)FS_MAX_PATHING_PROBES + 2 * kPathingMatrixBytes +
                                      (2 * sizeof(float) + sizeof(uint32_t)) * (size_t)FS_MAX_PATHING_PROBES;
PathingSet pathing_set(const fs_context* ctx) {
    PathingSet g{};
    char* b = ctx->pathing.d_block;
    g.probes = reinterpret_cast<const float4*>(b); b += sizeof(float4) * (size_t)FS_MAX_PATHING_PROBES;
    g.upper = reinterpret_cast<uint32_t*>(b); b += kPathingMatrixBytes;
    g.graph = reinterpret_cast<uint32_t*>(b); b += kPathingMatrixBytes;
    g.dL = reinterpret_cast<float*>(b); b += sizeof(float) * (size_t)FS_MAX_PATHING_PROBES;
    g.d = reinterpret_cast<float*>(b); b += sizeof(float) * (size_t)FS_MAX_PATHING_PROBES;
    g.pred = reinterpret_cast<uint32_t*>(b);
    g.n = (int32_t)(ctx->pathing.xyz.size() / 3);
    g.stride = 2 * ((g.n + 63) / 64);
    return g;
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
    if (!params_or_default(p, def, fs_direct_params_default)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_direct_params.struct_size mismatch");
    if (p->samples < 1 || p->samples > FS_MAX_DIRECT_SAMPLES || p->max_surfaces < 1 || p->max_surfaces > FS_DIRECT_MAX_QUERIES - 1 ||
        !finite_at_least_zero(p->source_radius) || !finite_at_least_zero(p->step) || !finite_at_least_zero(p->pullback) ||
        !finite_above_zero(p->dist_divisor) || !finite_above_zero(p->sound_speed))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad direct-path params");
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    PathStaging& st = ctx->direct_stage;
    { int gr = st.grow(ctx, count, PathLayout{{sizeof(float4), 0, 0, 0, 0, sizeof(fs_direct_path)}}, PathLayout{{0, 0, 0, 0, 0, sizeof(fs_direct_path)}});
      if (gr) return gr; }
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
    float4* h_src = reinterpret_cast<float4*>(st.host(kSegSources));
    fs_direct_path* h_out = reinterpret_cast<fs_direct_path*>(st.host(kSegOut));
    fs_direct_path* d_out = reinterpret_cast<fs_direct_path*>(st.dev(kSegOut));
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
    static const RowsPathsQuery<fs_reflection_params, ReflectKParams> q = {
        FS_MAX_REFLECTION_BATCH, "count out of range (1 .. FS_MAX_REFLECTION_BATCH)", "fs_reflection_params.struct_size mismatch",
        "bad reflection-path params", fs_reflection_params_default, &fs_context::reflect_stage,
        1, 0, FS_MAX_REFLECTION_CANDIDATES, 0, FS_MAX_REFLECTIONS, launch_reflection_paths};
    return update_rows_paths(q, ctx, sources, count, p, rows, paths, [](const fs_reflection_params& p) {
        return p.max_paths >= 1 && p.max_paths <= FS_MAX_REFLECTIONS && p.max_candidates >= 1 && p.max_candidates <= FS_MAX_REFLECTION_CANDIDATES &&
               finite_at_least_zero(p.margin) && finite_at_least_zero(p.step) && finite_at_least_zero(p.offset) && finite_at_least_zero(p.pullback) &&
               finite_above_zero(p.dist_divisor) && finite_above_zero(p.sound_speed);
    }, [](ReflectKParams& rp, const fs_reflection_params& p, const PathStaging& st) {
        rp.counters = staged_words(st, kSegCounters);
        rp.cand = staged_words(st, kSegCand);
        rp.max_candidates = p.max_candidates;
        rp.margin = p.margin;
        rp.offset = p.offset;
    });
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
    static const RowsPathsQuery<fs_diffraction_params, DiffractKParams> q = {
        FS_MAX_DIFFRACTION_BATCH, "count out of range (1 .. FS_MAX_DIFFRACTION_BATCH)", "fs_diffraction_params.struct_size mismatch",
        "bad diffraction-path params", fs_diffraction_params_default, &fs_context::diffract_stage,
        1, 0, FS_MAX_DIFFRACTION_CANDIDATES, sizeof(DiffractRecord), FS_MAX_DIFFRACTIONS, launch_diffraction_paths};
    return update_rows_paths(q, ctx, sources, count, p, rows, paths, [](const fs_diffraction_params& p) {
        return p.max_paths >= 1 && p.max_paths <= FS_MAX_DIFFRACTIONS && p.max_candidates >= 1 && p.max_candidates <= FS_MAX_DIFFRACTION_CANDIDATES &&
               finite_at_least_zero(p.margin) && finite_above_zero(p.max_detour) && finite_at_least_zero(p.offset) && finite_at_least_zero(p.merge) &&
               finite_at_least_zero(p.step) && finite_at_least_zero(p.pullback) && finite_above_zero(p.dist_divisor) && finite_above_zero(p.sound_speed);
    }, [ctx](DiffractKParams& dp, const fs_diffraction_params& p, const PathStaging& st) {
        dp.counters = staged_words(st, kSegCounters);
        dp.cand = staged_words(st, kSegCand);
        dp.conf = reinterpret_cast<DiffractRecord*>(st.dev(kSegConf));
        dp.max_candidates = p.max_candidates;
        dp.margin = p.margin;
        dp.max_detour = p.max_detour;
        dp.offset = p.offset;
        dp.merge = p.merge;
        band_factors(ctx, p.sound_speed, p.dist_divisor, dp.k, nullptr);
    });
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
    static const RowsPathsQuery<fs_reflection2_params, Reflect2KParams> q = {
        FS_MAX_REFLECTION2_BATCH, "count out of range (1 .. FS_MAX_REFLECTION2_BATCH)", "fs_reflection2_params.struct_size mismatch",
        "bad second-order reflection-path params", fs_reflection2_params_default, &fs_context::reflect2_stage,
        2, FS_MAX_REFLECTION2_NEAR, FS_MAX_REFLECTION2_CANDIDATES, sizeof(Reflect2Record), FS_MAX_REFLECTION2_PATHS, launch_reflection2_paths};
    return update_rows_paths(q, ctx, sources, count, p, rows, paths, [](const fs_reflection2_params& p) {
        return p.max_paths >= 1 && p.max_paths <= FS_MAX_REFLECTION2_PATHS && p.max_near >= 1 && p.max_near <= FS_MAX_REFLECTION2_NEAR &&
               p.max_candidates >= 1 && p.max_candidates <= FS_MAX_REFLECTION2_CANDIDATES && finite_above_zero(p.max_length) &&
               finite_at_least_zero(p.margin) && finite_at_least_zero(p.step) && finite_at_least_zero(p.offset) && finite_at_least_zero(p.pullback) &&
               finite_above_zero(p.dist_divisor) && finite_above_zero(p.sound_speed);
    }, [](Reflect2KParams& rp, const fs_reflection2_params& p, const PathStaging& st) {
        rp.l = staged_pair_lists(st, p.max_near, p.max_candidates);
        rp.conf = reinterpret_cast<Reflect2Record*>(st.dev(kSegConf));
        rp.max_length = p.max_length;
        rp.margin = p.margin;
        rp.offset = p.offset;
    });
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
    static const RowsPathsQuery<fs_diffraction2_params, Diffract2KParams> q = {
        FS_MAX_DIFFRACTION2_BATCH, "count out of range (1 .. FS_MAX_DIFFRACTION2_BATCH)", "fs_diffraction2_params.struct_size mismatch",
        "bad second-order diffraction-path params", fs_diffraction2_params_default, &fs_context::diffract2_stage,
        2, FS_MAX_DIFFRACTION2_NEAR, FS_MAX_DIFFRACTION2_CANDIDATES, sizeof(Diffract2Record), FS_MAX_DIFFRACTION2_PATHS, launch_diffraction2_paths};
    return update_rows_paths(q, ctx, sources, count, p, rows, paths, [](const fs_diffraction2_params& p) {
        return p.max_paths >= 1 && p.max_paths <= FS_MAX_DIFFRACTION2_PATHS && p.max_near >= 1 && p.max_near <= FS_MAX_DIFFRACTION2_NEAR &&
               p.max_candidates >= 1 && p.max_candidates <= FS_MAX_DIFFRACTION2_CANDIDATES && finite_at_least_zero(p.margin) &&
               finite_above_zero(p.max_detour) && finite_above_zero(p.min_parallel) && p.min_parallel <= 1.0f && finite_at_least_zero(p.offset) &&
               finite_at_least_zero(p.merge) && finite_at_least_zero(p.step) && finite_at_least_zero(p.pullback) &&
               finite_above_zero(p.dist_divisor) && finite_above_zero(p.sound_speed);
    }, [ctx](Diffract2KParams& dp, const fs_diffraction2_params& p, const PathStaging& st) {
        dp.l = staged_pair_lists(st, p.max_near, p.max_candidates);
        dp.conf = reinterpret_cast<Diffract2Record*>(st.dev(kSegConf));
        dp.margin = p.margin;
        dp.max_detour = p.max_detour;
        dp.min_parallel = p.min_parallel;
        dp.offset = p.offset;
        dp.merge = p.merge;
        band_factors(ctx, p.sound_speed, p.dist_divisor, dp.k, dp.lam5);
    });
}

// ---- mixed paths: one reflection and one edge diffraction --------------------------------------------------------------------
void fs_mixed_params_default(fs_mixed_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_mixed_params);
    p->max_paths = 8;
    p->max_near = 16384;
    p->max_candidates = 1024;
    p->max_length = 500.f;    // (at 750 a fifth of the old_mine rows overflow max_near, near counting a triangle up to four times: DESIGN.md "Mixed paths")
    p->max_detour = 1000.f;   // the first-order call's: here it bounds no list
    p->margin = 1e-3f;
    p->offset = 0.1f;
    p->merge = 1.0f;
    p->step = 0.1f;
    p->pullback = 0.1f;
    p->dist_divisor = 1000.f;
    p->sound_speed = 343.f;
}

int fs_update_mixed_paths(fs_context* ctx, const fs_source* sources, int32_t count, const fs_mixed_params* p, fs_mixed_row* rows,
                          fs_mixed_path* paths) {
    static const RowsPathsQuery<fs_mixed_params, MixedKParams> q = {
        FS_MAX_MIXED_BATCH, "count out of range (1 .. FS_MAX_MIXED_BATCH)", "fs_mixed_params.struct_size mismatch",
        "bad mixed-path params", fs_mixed_params_default, &fs_context::mixed_stage,
        2, FS_MAX_MIXED_NEAR, FS_MAX_MIXED_CANDIDATES, sizeof(MixedRecord), FS_MAX_MIXED_PATHS, launch_mixed_paths};
    return update_rows_paths(q, ctx, sources, count, p, rows, paths, [](const fs_mixed_params& p) {
        return p.max_paths >= 1 && p.max_paths <= FS_MAX_MIXED_PATHS && p.max_near >= 1 && p.max_near <= FS_MAX_MIXED_NEAR &&
               p.max_candidates >= 1 && p.max_candidates <= FS_MAX_MIXED_CANDIDATES && finite_above_zero(p.max_length) &&
               finite_above_zero(p.max_detour) && finite_at_least_zero(p.margin) && finite_at_least_zero(p.offset) &&
               finite_at_least_zero(p.merge) && finite_at_least_zero(p.step) && finite_at_least_zero(p.pullback) &&
               finite_above_zero(p.dist_divisor) && finite_above_zero(p.sound_speed);
    }, [ctx](MixedKParams& mp, const fs_mixed_params& p, const PathStaging& st) {
        mp.l = staged_pair_lists(st, p.max_near, p.max_candidates);
        mp.conf = reinterpret_cast<MixedRecord*>(st.dev(kSegConf));
        mp.max_length = p.max_length;
        mp.max_detour = p.max_detour;
        mp.margin = p.margin;
        mp.offset = p.offset;
        mp.merge = p.merge;
        band_factors(ctx, p.sound_speed, p.dist_divisor, mp.k, nullptr);
    });
}

// ---- pathing: round several corners by a probe graph -------------------------------------------------------------------------
void fs_pathing_bake_params_default(fs_pathing_bake_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_pathing_bake_params);
    p->max_edge = 1000.f;
    p->step = 0.1f;
}

void fs_pathing_params_default(fs_pathing_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_pathing_params);
    p->validate = 1;
    p->max_attach = 1000.f;
    p->max_length = 10000.f;
    p->step = 0.1f;
    p->pullback = 0.1f;
    p->dist_divisor = 1000.f;
    p->sound_speed = 343.f;
}

int fs_pathing_set_probes(fs_context* ctx, const float* xyz, int32_t count) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (count < 0 || count > FS_MAX_PATHING_PROBES) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (0 .. FS_MAX_PATHING_PROBES)");
    if (!xyz) count = 0;
    for (size_t i = 0; i < 3 * (size_t)count; ++i)
        if (!std::isfinite(xyz[i])) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "non-finite probe coordinate");
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    fs_context::Pathing& pa = ctx->pathing;
    if (count > 0) {
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        if (!pa.d_block) FS_HIP(ctx, hipMalloc((void**)&pa.d_block, kPathingBlockBytes));
        std::vector<float4> packed((size_t)count);
        for (int32_t k = 0; k < count; ++k) packed[(size_t)k] = make_float4(xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2], 0.0f);
        // (every earlier call has been waited for: nothing in the stream reads the old probes)
        FS_HIP(ctx, hipMemcpy(pa.d_block, packed.data(), sizeof(float4) * (size_t)count, hipMemcpyHostToDevice));
    }
    pa.xyz.assign(xyz, xyz + 3 * (size_t)count);
    pa.graph.clear();
    pa.edges = 0;
    pa.baked = false;
    return FS_OK;
}

int fs_pathing_bake(fs_context* ctx, const fs_pathing_bake_params* p) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    fs_pathing_bake_params def;
    if (!params_or_default(p, def, fs_pathing_bake_params_default)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_pathing_bake_params.struct_size mismatch");
    if (!finite_above_zero(p->max_edge) || !finite_at_least_zero(p->step)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad pathing bake params");
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    fs_context::Pathing& pa = ctx->pathing;
    if (pa.xyz.empty()) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "no probes (fs_pathing_set_probes)");
    { int pr = paths_prologue(ctx, nullptr, 0); if (pr) return pr; }
    PathingBakeKParams bp{};
    bp.h.lis_object = FS_NO_OBJECT;
    bp.h.num_bands = ctx->cfg.num_bands;
    bp.h.step = p->step;
    bp.g = pathing_set(ctx);
    bp.max_edge = p->max_edge;
    const int n = bp.g.n, words = (n + 31) / 32;
    pa.baked = false;
    std::vector<uint32_t> wide((size_t)n * (size_t)bp.g.stride);
    launch_pathing_bake(ctx->scene, bp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipMemcpyAsync(wide.data(), bp.g.graph, sizeof(uint32_t) * wide.size(), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pa.graph.resize((size_t)n * (size_t)words);
    size_t bits = 0;
    for (int i = 0; i < n; ++i)
        for (int w = 0; w < words; ++w) {
            const uint32_t v = wide[(size_t)i * (size_t)bp.g.stride + (size_t)w];
            pa.graph[(size_t)i * (size_t)words + (size_t)w] = v;
            bits += (size_t)__builtin_popcount(v);
        }
    pa.edges = (int32_t)(bits / 2);
    pa.baked = true;
    pa.baked_gen = ctx->scene_gen;
    return FS_OK;
}

int fs_pathing_info(fs_context* ctx, int32_t* probes, int32_t* edges, int32_t* baked, int32_t* scene_changed) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    const fs_context::Pathing& pa = ctx->pathing;
    if (probes) *probes = (int32_t)(pa.xyz.size() / 3);
    if (edges) *edges = pa.baked ? pa.edges : 0;
    if (baked) *baked = pa.baked ? 1 : 0;
    if (scene_changed) *scene_changed = pa.baked && pa.baked_gen != ctx->scene_gen ? 1 : 0;
    return FS_OK;
}

int fs_pathing_copy_graph(fs_context* ctx, uint32_t* bits, int32_t words) {
    if (!ctx || !bits) return FS_ERR_INVALID_ARGUMENT;
    const fs_context::Pathing& pa = ctx->pathing;
    if (!pa.baked) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "no baked graph (fs_pathing_bake)");
    if (words < 0 || (size_t)words != pa.graph.size()) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "words is not N ceil(N / 32)");
    std::memcpy(bits, pa.graph.data(), sizeof(uint32_t) * pa.graph.size());
    return FS_OK;
}

int fs_update_pathing_paths(fs_context* ctx, const fs_source* sources, int32_t count, const fs_pathing_params* p, fs_pathing_path* out) {
    if (!ctx || !sources || !out) return FS_ERR_INVALID_ARGUMENT;
    if (count < 1 || count > FS_MAX_PATHING_BATCH) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_PATHING_BATCH)");
    fs_pathing_params def;
    if (!params_or_default(p, def, fs_pathing_params_default)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_pathing_params.struct_size mismatch");
    if ((p->validate != 0 && p->validate != 1) || !finite_above_zero(p->max_attach) ||!finite_above_zero(p->max_length) || p->max_length > FS_PATHING_MAX_LENGTH ||
        !finite_at_least_zero(p->step) || !finite_at_least_zero(p->pullback) || !finite_above_zero(p->dist_divisor) || !finite_above_zero(p->sound_speed))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad pathing params");
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (!ctx->pathing.baked) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "no baked graph (fs_pathing_bake)");
    { int pr = paths_prologue(ctx, sources, count); if (pr) return pr; }
    PathStaging& st = ctx->pathing_stage;
    const PathLayout layout{{sizeof(float4), 0, 0, 0, 0, sizeof(fs_pathing_path)}};
    { int gr = st.grow(ctx, count, layout, layout); if (gr) return gr; }
    float4* h_src = reinterpret_cast<float4*>(st.host(kSegSources));
    float4* d_src = reinterpret_cast<float4*>(st.dev(kSegSources));
    fs_pathing_path* h_out = reinterpret_cast<fs_pathing_path*>(st.host(kSegOut));
    fs_pathing_path* d_out = reinterpret_cast<fs_pathing_path*>(st.dev(kSegOut));
    pack_sources(ctx, sources, count, h_src);
    PathingKParams pp{};
    pp.h = path_head(ctx, d_src, count, p->step, p->pullback, p->dist_divisor, p->sound_speed);
    pp.g = pathing_set(ctx);
    pp.out = d_out;
    pp.validate = p->validate;
    pp.max_attach = p->max_attach;
    pp.max_length = p->max_length;
    band_factors(ctx, p->sound_speed, p->dist_divisor, pp.k, nullptr);
    FS_HIP(ctx, hipMemcpyAsync(d_src, h_src, sizeof(float4) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    launch_pathing_paths(ctx->scene, pp, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipMemcpyAsync(h_out, d_out, sizeof(fs_pathing_path) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, h_out, sizeof(fs_pathing_path) * (size_t)count);
    return FS_OK;
}

}  // extern "C"
