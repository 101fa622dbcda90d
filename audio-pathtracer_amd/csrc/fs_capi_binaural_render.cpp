// fs_capi_binaural_render.cpp — binaural voices on the audio thread: the HRIR set of the context (fs_hrtf_set / fs_hrtf_info), a
// set for hosts that have none (fs_hrtf_spherical_head, host only), the mesh on the set that turns the nearest direction into a
// blend of three (fs_hrtf_triangulate, fs_hrtf_mesh_rows, fs_hrtf_mesh_locate: host only; fs_hrtf_set_mesh / fs_hrtf_mesh_info),
// the onsets on the set that turn the blend of HRIRs into a blend of aligned HRIRs and of their delays (fs_hrtf_delay,
// fs_hrtf_split_onsets, fs_hrtf_spherical_head_split: host only; fs_hrtf_set_onsets / fs_hrtf_onsets_info),
// and what the renderer is beyond its voice bank
// (fs_capi_voice_bank.hpp: the callback; fs_capi_reflect_render.cpp: the set-up and its release): the refusals that name the
// set, an entry's gain and direction, the list of sounding slots and the folded tables of fs_binaural_render.hip's launches.
// The band kernels and their per-context cache are the direct renderer's (fs_capi_direct_render.cpp).  The reference has no slot
// for it.
#include <algorithm>

#include "fs_capi_voice_bank.hpp"

static_assert(sizeof(fs_binaural_voice) == 56, "fs_binaural_voice: the key, the delay, the bands, the gain, the direction");
static_assert(sizeof(fs_binaural_render_row) == 16, "fs_binaural_render_row: four counts");
static_assert(FS_MAX_REFLECTION_RENDER_BATCH * FS_MAX_REFLECTION_VOICES <= 65536, "BinauralRenderBatch::sounding: 16 bits per (row, slot)");

namespace {

constexpr double kPi = 3.14159265358979323846;

// the header's spherical-head model for one ear at angle theta from the ear's axis, in double: the onset tau and the shadow
// filter's b0, b1, a1 ...
struct HeadEar { double tau, b0, b1, a1; };
HeadEar head_ear(double theta, double a_over_c, double fs) {
    const double tau = theta <= kPi / 2.0 ? a_over_c * (1.0 - std::cos(theta)) : a_over_c * (1.0 + theta - kPi / 2.0);
    const double alpha_min = 0.1, theta_min = 5.0 * kPi / 6.0;
    const double alpha = (1.0 + alpha_min / 2.0) + (1.0 - alpha_min / 2.0) * std::cos(theta * kPi / theta_min);
    const double kappa = fs * a_over_c;
    return {tau, (1.0 + alpha * kappa) / (1.0 + kappa), (1.0 - alpha * kappa) / (1.0 + kappa), (1.0 - kappa) / (1.0 + kappa)};
}
// ... its taps h[0 .. H) ...
void head_taps(double theta, double a_over_c, double fs, int H, double* h) {
    const HeadEar e = head_ear(theta, a_over_c, fs);
    const double tau = e.tau, b0 = e.b0, b1 = e.b1, a1 = e.a1;
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
// ... and the two halves apart (fs_hrtf_spherical_head_split): g[0 .. H), the shadow filter alone
void head_filter(const HeadEar& e, int H, double* g) {
    for (int m = 0; m < H; ++m) g[m] = m == 0 ? e.b0 : m == 1 ? e.b1 - e.a1 * g[0] : -e.a1 * g[m - 1];
}

// fs_hrtf_spherical_head (onsets == nullptr) and fs_hrtf_spherical_head_split: the directions, and per ear the taps — with the
// onset in them, or beside them
int spherical_head(int32_t sample_rate, float radius_cm, float sound_speed_cm_s, int32_t directions, int32_t taps, float* dirs, float* hrir,
                   float* onsets, bool split) {
    if (!dirs || !hrir || (split && !onsets) || sample_rate < 1 || !std::isfinite(radius_cm) || !(radius_cm > 0.0f) ||
        !std::isfinite(sound_speed_cm_s) || !(sound_speed_cm_s > 0.0f) || directions < 1 || directions > FS_MAX_HRTF_DIRECTIONS ||
        taps < (split ? 2 : 1) || taps > FS_MAX_HRTF_TAPS)
        return FS_ERR_INVALID_ARGUMENT;
    const double fs = (double)sample_rate, a_over_c = (double)radius_cm / (double)sound_speed_cm_s;
    if (!split && (double)taps < std::ceil(a_over_c * (1.0 + kPi / 2.0) * fs) + 2.0) return FS_ERR_INVALID_ARGUMENT;
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
            if (split) {
                const HeadEar e = head_ear(theta, a_over_c, fs);
                head_filter(e, H, h.data());
                onsets[(size_t)k * 2 + (size_t)ear] = (float)(e.tau * fs);
            } else {
                head_taps(theta, a_over_c, fs, H, h.data());
            }
            float* out = hrir + ((size_t)k * 2 + (size_t)ear) * (size_t)H;
            for (int t = 0; t < H; ++t) out[t] = (float)h[(size_t)t];
        }
    }
    return FS_OK;
}

// ---- the mesh on a set: the header's "fs_hrtf_mesh_rows" clauses, in double from the float directions as given.  True: the mesh
// is accepted and rows [m][3][3] (when not null) holds r_0, r_1, r_2 of every triangle, each component rounded to float once.
bool mesh_rows(const float* dirs, int n, const int32_t* tri, int m, float* rows) {
    if (!dirs || !tri || n < 4 || n > FS_MAX_HRTF_DIRECTIONS || m != 2 * n - 4) return false;
    std::vector<int64_t> edges((size_t)m * 3);
    std::vector<char> used((size_t)n, 0);
    for (int j = 0; j < m; ++j) {
        const int32_t* t = tri + (size_t)j * 3;
        for (int i = 0; i < 3; ++i)
            if (t[i] < 0 || t[i] >= n) return false;
        if (t[0] == t[1] || t[1] == t[2] || t[2] == t[0]) return false;
        for (int i = 0; i < 3; ++i) {
            used[(size_t)t[i]] = 1;
            edges[(size_t)j * 3 + (size_t)i] = (int64_t)t[i] * n + t[(i + 1) % 3];
        }
    }
    for (int k = 0; k < n; ++k)
        if (!used[(size_t)k]) return false;
    std::sort(edges.begin(), edges.end());
    if (std::adjacent_find(edges.begin(), edges.end()) != edges.end()) return false;   // a directed edge in two triangles
    for (const int64_t e : edges)
        if (!std::binary_search(edges.begin(), edges.end(), (e % n) * n + e / n)) return false;   // ... or without its reverse
    std::vector<float> out(rows ? (size_t)m * 9 : 0);
    for (int j = 0; j < m; ++j) {
        double p[3][3];
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) p[i][c] = (double)dirs[(size_t)tri[(size_t)j * 3 + (size_t)i] * 3 + (size_t)c];
        double x[3][3];   // x[i] = p[i + 1] x p[i + 2]
        for (int i = 0; i < 3; ++i) {
            const double* a = p[(i + 1) % 3];
            const double* b = p[(i + 2) % 3];
            x[i][0] = a[1] * b[2] - a[2] * b[1];
            x[i][1] = a[2] * b[0] - a[0] * b[2];
            x[i][2] = a[0] * b[1] - a[1] * b[0];
        }
        const double det = p[0][0] * x[0][0] + p[0][1] * x[0][1] + p[0][2] * x[0][2];
        if (!(det >= 1e-6) || !std::isfinite(det)) return false;
        if (rows)
            for (int i = 0; i < 3; ++i)
                for (int c = 0; c < 3; ++c) out[((size_t)j * 3 + (size_t)i) * 3 + (size_t)c] = (float)(x[i][c] / det);
    }
    if (rows) std::memcpy(rows, out.data(), sizeof(float) * out.size());
    return true;
}

// The convex hull of n points in double, incrementally with brute-force visibility: a tetrahedron of four points far apart, then
// every other point in index order — the faces whose plane it lies above by more than kHullEps go, and the rim they leave (the
// directed edges whose reverse is not among them) is joined to the point.  A point within kHullEps of a face's plane leaves the
// face in place and extends its facet in that plane: co-circular directions (a lat-long grid, a cube) split their facet one way or
// another.  tri [2n - 4][3]; false when no tetrahedron is found or the faces do not come to 2n - 4 (mesh_rows judges the rest).
constexpr double kHullEps = 1e-12;
struct HullFace { int v[3]; double n[3], off; };   // unit normal, n . x = off on the plane
bool hull_face(const double* pts, int a, int b, int c, HullFace* f) {
    const double *pa = pts + 3 * (size_t)a, *pb = pts + 3 * (size_t)b, *pc = pts + 3 * (size_t)c;
    const double u[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]}, w[3] = {pc[0] - pa[0], pc[1] - pa[1], pc[2] - pa[2]};
    double nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
    const double len = std::sqrt(nx * nx + ny * ny + nz * nz);
    if (!(len > 0.0)) return false;
    nx /= len; ny /= len; nz /= len;
    *f = {{a, b, c}, {nx, ny, nz}, nx * pa[0] + ny * pa[1] + nz * pa[2]};
    return true;
}
inline double hull_height(const HullFace& f, const double* p) { return f.n[0] * p[0] + f.n[1] * p[1] + f.n[2] * p[2] - f.off; }
bool convex_hull(const double* pts, int n, int32_t* tri) {
    auto dist2 = [&](int a, int b) {
        double s = 0.0;
        for (int c = 0; c < 3; ++c) { const double d = pts[3 * (size_t)a + c] - pts[3 * (size_t)b + c]; s += d * d; }
        return s;
    };
    int i0 = 0, i1 = 0, i2 = -1, i3 = -1;
    for (int k = 1; k < n; ++k)
        if (dist2(0, k) > dist2(0, i1)) i1 = k;
    if (i1 == 0) return false;
    double best = 0.0;
    HullFace f;
    for (int k = 0; k < n; ++k) {   // the widest triangle on (i0, i1)
        if (k == i0 || k == i1 || !hull_face(pts, i0, i1, k, &f)) continue;
        const double *pa = pts + 3 * (size_t)i0, *pb = pts + 3 * (size_t)i1, *pc = pts + 3 * (size_t)k;
        const double u[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]}, w[3] = {pc[0] - pa[0], pc[1] - pa[1], pc[2] - pa[2]};
        const double cx = u[1] * w[2] - u[2] * w[1], cy = u[2] * w[0] - u[0] * w[2], cz = u[0] * w[1] - u[1] * w[0];
        const double area2 = cx * cx + cy * cy + cz * cz;
        if (area2 > best) { best = area2; i2 = k; }
    }
    if (i2 < 0 || !(best > 1e-12) || !hull_face(pts, i0, i1, i2, &f)) return false;
    best = 0.0;
    for (int k = 0; k < n; ++k) {   // the point farthest from its plane
        const double h = std::fabs(hull_height(f, pts + 3 * (size_t)k));
        if (h > best) { best = h; i3 = k; }
    }
    if (i3 < 0 || !(best > 1e-9)) return false;   // (all in one plane: a great circle)
    if (hull_height(f, pts + 3 * (size_t)i3) > 0.0) std::swap(i1, i2);   // (i0, i1, i2) seen counter-clockwise from outside: i3 below
    std::vector<HullFace> faces;
    faces.reserve((size_t)2 * (size_t)n);
    const int first[4][3] = {{i0, i1, i2}, {i0, i3, i1}, {i1, i3, i2}, {i2, i3, i0}};
    for (const auto& t : first) {
        if (!hull_face(pts, t[0], t[1], t[2], &f)) return false;
        faces.push_back(f);
    }
    std::vector<int64_t> rim, gone;
    for (int k = 0; k < n; ++k) {
        if (k == i0 || k == i1 || k == i2 || k == i3) continue;
        const double* p = pts + 3 * (size_t)k;
        gone.clear();
        size_t kept = 0;
        for (size_t j = 0; j < faces.size(); ++j) {
            if (hull_height(faces[j], p) > kHullEps) {
                for (int i = 0; i < 3; ++i) gone.push_back((int64_t)faces[j].v[i] * n + faces[j].v[(i + 1) % 3]);
            } else {
                faces[kept++] = faces[j];
            }
        }
        if (gone.empty()) continue;   // inside or on the hull so far: left out (a duplicate; mesh_rows will miss it)
        faces.resize(kept);
        std::sort(gone.begin(), gone.end());
        rim.clear();
        for (const int64_t e : gone)
            if (!std::binary_search(gone.begin(), gone.end(), (e % n) * n + e / n)) rim.push_back(e);
        for (const int64_t e : rim) {
            if (!hull_face(pts, (int)(e / n), (int)(e % n), k, &f)) return false;
            faces.push_back(f);
        }
    }
    if (faces.size() != (size_t)(2 * n - 4)) return false;
    for (size_t j = 0; j < faces.size(); ++j)
        for (int i = 0; i < 3; ++i) tri[j * 3 + (size_t)i] = faces[j].v[i];
    return true;
}

// what fs_hrtf_set and fs_hrtf_set_mesh do to the voices: every held slot is free, on both copies of the slot tables; the rings and
// the counters stay.  The host's copies — what the matching reads, so every voice starts — all go first, and a failed clear of a
// device copy (which a start overwrites anyway) is reported only after every source has had its turn.
hipError_t free_binaural_slots(fs_context* ctx) {
    for (Source* s : ctx->sources)
        if (s && s->alive && s->br.r.d) s->br.free_slots();
    hipError_t clear_err = hipSuccess;
    for (Source* s : ctx->sources) {
        if (!s || !s->alive || !s->br.r.d) continue;
        const hipError_t e = hipMemsetAsync(s->br.r.d + offsetof(BinauralRenderState, slot), 0, sizeof(BinauralRenderState::slot), ctx->rev_stream);
        if (e != hipSuccess && clear_err == hipSuccess) clear_err = e;
    }
    return clear_err;
}

}  // namespace

extern "C" {

int fs_hrtf_spherical_head(int32_t sample_rate, float radius_cm, float sound_speed_cm_s, int32_t directions, int32_t taps, float* dirs,
                           float* hrir) {
    return spherical_head(sample_rate, radius_cm, sound_speed_cm_s, directions, taps, dirs, hrir, nullptr, false);
}

int fs_hrtf_spherical_head_split(int32_t sample_rate, float radius_cm, float sound_speed_cm_s, int32_t directions, int32_t taps, float* dirs,
                                 float* hrir, float* onsets) {
    return spherical_head(sample_rate, radius_cm, sound_speed_cm_s, directions, taps, dirs, hrir, onsets, true);
}

int fs_hrtf_delay(const float* h, int32_t H, float tau, float* out, int32_t He) {
    if (!h || !out || H < 1 || !std::isfinite(tau) || !(tau >= 0.0f) || tau >= 2147483520.0f || (int64_t)He < (int64_t)H + (int64_t)tau + 1)
        return FS_ERR_INVALID_ARGUMENT;
    const HrtfDelay d = hrtf_delay_of(tau);
    for (int k = 0; k < He; ++k) out[k] = hrtf_delay_tap(d, k, [=](int j) { return j >= 0 && j < H ? h[j] : 0.0f; });
    return FS_OK;
}

int fs_hrtf_split_onsets(const float* hrir, int32_t n, int32_t H, float threshold, int32_t lead, float* aligned, float* onsets) {
    if (!hrir || !aligned || !onsets || n < 1 || H < 1 || !(threshold > 0.0f) || !(threshold <= 1.0f) || lead < 0) return FS_ERR_INVALID_ARGUMENT;
    for (size_t r = 0; r < (size_t)n * 2; ++r) {
        const float* h = hrir + r * (size_t)H;
        float* a = aligned + r * (size_t)H;
        float peak = 0.0f;
        for (int k = 0; k < H; ++k) peak = std::max(peak, std::fabs(h[k]));
        const float level = threshold * peak;
        int k0 = 0;
        while (k0 < H && !(std::fabs(h[k0]) >= level)) ++k0;
        if (k0 == H) k0 = 0;   // (taps that are not numbers)
        const int onset = std::max(k0 - std::min(lead, k0), 0);
        for (int k = 0; k < H; ++k) a[k] = k + onset < H ? h[k + onset] : 0.0f;   // (ascending: in place reads ahead of what it writes)
        onsets[r] = (float)onset;
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
    if (d) ctx->hrtf_dirs_host.assign(d->dirs, d->dirs + n_dir); else ctx->hrtf_dirs_host.clear();
    if (ctx->d_hrtf_mesh) (void)hipFree(ctx->d_hrtf_mesh);   // a mesh is of the set it was given for
    ctx->d_hrtf_mesh = nullptr;
    ctx->hrtf_tris = 0;
    if (ctx->d_hrtf_onsets) (void)hipFree(ctx->d_hrtf_onsets);   // ... and so are onsets
    ctx->d_hrtf_onsets = nullptr;
    ctx->hrtf_omax = 0.0f;
    ctx->hrtf_onset_taps = 0;
    // The set is in force from here on, so no source is left out
    const hipError_t clear_err = free_binaural_slots(ctx);
    if (clear_err != hipSuccess) return ctx->hip_fail(clear_err, "fs_hrtf_set (clearing the slots)");
    return FS_OK;
}

int fs_hrtf_triangulate(const float* dirs, int32_t n, int32_t* tri, int32_t cap, int32_t* m) {
    if (!dirs || !tri || !m || n < 4 || n > FS_MAX_HRTF_DIRECTIONS || cap < 2 * n - 4) return FS_ERR_INVALID_ARGUMENT;
    std::vector<double> pts((size_t)n * 3);
    for (size_t k = 0; k < pts.size(); ++k) {
        if (!std::isfinite(dirs[k])) return FS_ERR_INVALID_ARGUMENT;
        pts[k] = (double)dirs[k];
    }
    std::vector<int32_t> faces((size_t)(2 * n - 4) * 3);
    if (!convex_hull(pts.data(), n, faces.data()) || !mesh_rows(dirs, n, faces.data(), 2 * n - 4, nullptr)) return FS_ERR_INVALID_ARGUMENT;
    std::memcpy(tri, faces.data(), sizeof(int32_t) * faces.size());
    *m = 2 * n - 4;
    return FS_OK;
}

int fs_hrtf_mesh_rows(const float* dirs, int32_t n, const int32_t* tri, int32_t m, float* rows) {
    return mesh_rows(dirs, n, tri, m, rows) ? FS_OK : FS_ERR_INVALID_ARGUMENT;
}

int fs_hrtf_mesh_locate(const float* rows, int32_t m, const float d[3], int32_t* t, float b[3]) {
    if (!rows || !d || !t || !b || m < 1) return FS_ERR_INVALID_ARGUMENT;
    const HrtfMeshRowsHost r = {rows};
    const HrtfMeshBest best = hrtf_mesh_scan(r, m, d, 0, 1);
    *t = best.j;
    hrtf_mesh_weights(r, best.j, d, b);
    return FS_OK;
}

int fs_hrtf_set_mesh(fs_context* ctx, const int32_t* tri, int32_t m) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (ctx->hrtf_dirs == 0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set_mesh: no HRIR set in force (fs_hrtf_set)");
    const bool clear = !tri || m == 0;
    std::vector<float4> block;
    if (!clear) {
        std::vector<float> rows((size_t)(m > 0 ? m : 0) * 9);
        if (m < 0 || !mesh_rows(ctx->hrtf_dirs_host.data(), ctx->hrtf_dirs, tri, m, rows.data()))
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set_mesh: not a closed, outward-facing triangulation of the set's directions (fs_hrtf_mesh_rows)");
        block.resize((size_t)m * 3);
        for (size_t k = 0; k < block.size(); ++k) {
            float4& q = block[k];
            q.x = rows[k * 3]; q.y = rows[k * 3 + 1]; q.z = rows[k * 3 + 2];
            const uint32_t v = (uint32_t)tri[k];
            std::memcpy(&q.w, &v, sizeof(v));
        }
    }
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    float4* fresh = nullptr;
    if (!clear) FS_HIP(ctx, hipMalloc((void**)&fresh, sizeof(float4) * block.size()));   // (a failure here has changed nothing)
    hipError_t err = hipStreamSynchronize(ctx->rev_stream);   // no callback reads the old mesh any more
    if (err == hipSuccess && !clear) err = hipMemcpy(fresh, block.data(), sizeof(float4) * block.size(), hipMemcpyHostToDevice);
    if (err != hipSuccess) { if (fresh) (void)hipFree(fresh); return ctx->hip_fail(err, "fs_hrtf_set_mesh (upload)"); }
    if (ctx->d_hrtf_mesh) (void)hipFree(ctx->d_hrtf_mesh);
    ctx->d_hrtf_mesh = fresh;
    ctx->hrtf_tris = clear ? 0 : m;
    const hipError_t clear_err = free_binaural_slots(ctx);   // nothing ramps from an index of the other mode
    if (clear_err != hipSuccess) return ctx->hip_fail(clear_err, "fs_hrtf_set_mesh (clearing the slots)");
    return FS_OK;
}

int fs_hrtf_mesh_info(fs_context* ctx, int32_t* triangles) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (triangles) *triangles = ctx->hrtf_tris;
    return FS_OK;
}

int fs_hrtf_set_onsets(fs_context* ctx, const float* onsets) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (ctx->hrtf_dirs == 0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set_onsets: no HRIR set in force (fs_hrtf_set)");
    const size_t count = (size_t)ctx->hrtf_dirs * 2;
    float omax = 0.0f;
    int extra = 0;
    if (onsets) {
        for (size_t k = 0; k < count; ++k) {
            if (!std::isfinite(onsets[k]) || !(onsets[k] >= 0.0f))
                return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set_onsets: an onset is not finite or is negative");
            omax = std::max(omax, onsets[k]);
        }
        if (!(omax < (float)FS_MAX_HRTF_TAPS) || ctx->hrtf_taps + (int)omax + 1 > FS_MAX_HRTF_TAPS)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_hrtf_set_onsets: the set's taps + (int) the largest onset + 1 exceed 512");
        extra = (int)omax + 1;
    }
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    float* fresh = nullptr;
    if (onsets) FS_HIP(ctx, hipMalloc((void**)&fresh, sizeof(float) * count));   // (a failure here has changed nothing)
    hipError_t err = hipStreamSynchronize(ctx->rev_stream);   // no callback reads the old onsets any more
    if (err == hipSuccess && onsets) err = hipMemcpy(fresh, onsets, sizeof(float) * count, hipMemcpyHostToDevice);
    if (err != hipSuccess) { if (fresh) (void)hipFree(fresh); return ctx->hip_fail(err, "fs_hrtf_set_onsets (upload)"); }
    if (ctx->d_hrtf_onsets) (void)hipFree(ctx->d_hrtf_onsets);
    ctx->d_hrtf_onsets = fresh;
    ctx->hrtf_omax = omax;
    ctx->hrtf_onset_taps = extra;
    const hipError_t clear_err = free_binaural_slots(ctx);   // nothing ramps from a table of the other length
    if (clear_err != hipSuccess) return ctx->hip_fail(clear_err, "fs_hrtf_set_onsets (clearing the slots)");
    return FS_OK;
}

int fs_hrtf_onsets_info(fs_context* ctx, int32_t* installed, int32_t* extra_taps) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (installed) *installed = ctx->d_hrtf_onsets ? 1 : 0;
    if (extra_taps) *extra_taps = ctx->hrtf_onset_taps;
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
    return voice_bank_init(ctx, h, &Source::br, ctx->hrtf_dirs ? ctx->hrtf_taps + ctx->hrtf_onset_taps - 1 : -1,   // (He - 1)
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
    const int H = ctx ? ctx->hrtf_taps + ctx->hrtf_onset_taps : 0;   // He: the taps of the HRIRs the fold runs on
    const bool mesh = ctx && ctx->hrtf_tris > 0;
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
        // allocates once), with a mesh followed by its plans and what the locate pass finds, [count][kVoiceSlots] each
        [&](size_t slots, const RenderSetup& shape) {
            const size_t folded = sizeof(float2) * slots * 2 * (size_t)(shape.taps + H - 1);
            const size_t located = mesh ? (sizeof(BinauralMeshPlan) + sizeof(float4)) * (size_t)count * kVoiceSlots : 0;
            return std::array<size_t, 3>{sizeof(uint16_t) * slots, (folded + 15) / 16 * 16 + located, 2 * (size_t)shape.frame};
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
            b.n_dirs = ctx->hrtf_dirs; b.h_taps = ctx->hrtf_taps; b.h_eff = H;
            b.onsets = ctx->d_hrtf_onsets; b.omax = ctx->hrtf_omax;
            b.tc = b.taps + H - 1;
            if (mesh) {
                size_t slots = 0;
                for (int i = 0; i < b.count; ++i) slots += (size_t)items[i].slots;
                char* behind = d_folded + (sizeof(float2) * slots * 2 * (size_t)b.tc + 15) / 16 * 16;
                b.mesh_plans = (BinauralMeshPlan*)behind;
                b.located = (float4*)(behind + sizeof(BinauralMeshPlan) * (size_t)b.count * kVoiceSlots);
                b.mesh = ctx->d_hrtf_mesh;
                b.n_tris = ctx->hrtf_tris;
            }
        });
}

}  // extern "C"
