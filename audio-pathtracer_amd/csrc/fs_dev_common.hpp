// fs_dev_common.hpp — device-side code of the FrequenSee BDPT path that every stage shares (gfx950, wave64): the
// namespace constants, the diagnostic builds' device globals, the RNG and sampling maps, ray / triangle arithmetic and
// the per-band segment term of EvaluatePath.  The stages build on it: fs_dev_trav.hpp (BVH traversal, wave work
// sharing), fs_dev_walk.hpp (walker, segment records, plan pass, walk bodies), fs_dev_coop.hpp (cooperative traversal),
// fs_dev_connect.hpp (connect pass), fs_dev_recon.hpp (reconstruct, publish); fs_launch.hpp holds the host-side launch
// helpers.  Everything is inline in an anonymous namespace: fs_walk.hip, fs_connect.hip, fs_frame.hip and
// fs_aux_kernels.hip each instantiate the kernels they launch (built side by side; fs_kernels_all.hip is the same code as
// one unit for the diagnostic builds, whose device-side debug symbols must be shared by all kernels).
//
// The triangle test, the hit point/normal/offset arithmetic and the sampling maps use a fixed
// operation order with explicit fmaf and are compiled with -ffp-contract=off: the path geometry is a
// pure function of (scene, seed, pair index) and does not depend on launch geometry or on the BVH.
#pragma once
#include <algorithm>
#include <atomic>

#include "fs_internal.hpp"

namespace fs {
namespace {

constexpr float kPi = 3.1415926535897932f;
constexpr uint32_t kNoMat = FS_NO_MATERIAL;
constexpr uint32_t kLobeDiffuse = 0u, kLobeSpecular = 1u, kLobeTransmit = 2u;
constexpr int kLobeShift = 16;   // segment record: material id | lobe << 16
constexpr int kDone = (int)0x80000000;  // traversal cursor: nothing left
constexpr double kFixedScale = 1099511627776.0;   // 2^40: quantum of the deterministic (fixed-point) energy sum
#ifdef FS_WAVE_TIMELINE   // diagnostic build only (tools/wave_timeline.py): when every walk wave ran and what it spent its cycles on
__device__ unsigned long long* g_wave_buf;       // [waves][8]: start, end (100 MHz), cycles in traversal, cycles in all, iterations, segments, hw id, slot
__device__ unsigned long long* g_conn_buf;       // [waves][8]: connect kernel: start, set-up done, visibility done, evaluated, end (100 MHz), lane-0 deposits
#endif
#ifdef FS_TRAV_STATS
__device__ unsigned long long g_trav_stats[32];  // closest-hit queries at [0..15], any-hit at [16..31]: [0] step calls, [1] node iterations,
                                                 // [2] node lanes, [3] tri iterations, [4] tri lanes, [5..7] node visits by children hit,
                                                 // [8] busy lanes, [9] lanes on taken work, [10] sharing-loop iterations, [11] lanes with both kinds
__device__ unsigned short* g_step_buf;           // optional [depth][2P]: traversal iterations of every walk segment
#endif

// ---------------------------------------------------------------------------------------------------
// RNG: Philox4x32-10, counter = (pair, bounce<<1|side, block, 'FS01'), key = seed
// ---------------------------------------------------------------------------------------------------
// (legacy tracer: counter = (ray, 0, 0, 'FS02'))
__device__ __forceinline__ uint4 philox(uint32_t pair, uint32_t bs, uint32_t block, uint32_t k0, uint32_t k1,
                                        uint32_t domain = 0x46533031u) {
    uint32_t c0 = pair, c1 = bs, c2 = block, c3 = domain;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-08f; }

// sin/cos(2 pi u): quadrant reduction + fixed fmaf polynomials (bit-reproducible, unlike sinf/cosf)
__device__ __forceinline__ void sincos2pi(float u, float& s_out, float& c_out) {
    float q = floorf(fmaf(u, 4.0f, 0.5f));
    float a = fmaf(q, -0.25f, u);
    float x = a * 6.283185307179586f;
    float x2 = x * x;
    float sp = 2.7557319e-06f;
    sp = fmaf(sp, x2, -1.9841270e-04f);
    sp = fmaf(sp, x2, 8.3333333e-03f);
    sp = fmaf(sp, x2, -1.6666667e-01f);
    float s = fmaf(sp * x2, x, x);
    float cp = 2.4801587e-05f;
    cp = fmaf(cp, x2, -1.3888889e-03f);
    cp = fmaf(cp, x2, 4.1666667e-02f);
    cp = fmaf(cp, x2, -0.5f);
    float c = fmaf(cp, x2, 1.0f);
    int k = ((int)q) & 3;
    s_out = (k == 0) ? s : (k == 1) ? c : (k == 2) ? -s : -c;
    c_out = (k == 0) ? c : (k == 1) ? -s : (k == 2) ? -c : s;
}

// FMath::VRand: cube rejection until 1e-4 < |v|^2 <= 1, normalise (ARTS.cpp:308)
__device__ __forceinline__ void sample_sphere(uint32_t pair, uint32_t bs, uint4 r0, uint32_t k0, uint32_t k1,
                                              float& dx, float& dy, float& dz) {
    uint32_t a = r0.y, b = r0.z, c = r0.w;
    dx = 0.f; dy = 0.f; dz = 1.f;
    for (uint32_t attempt = 0; attempt < 16; ++attempt) {
        if (attempt > 0) {
            uint4 r = philox(pair, bs, attempt, k0, k1);
            a = r.x; b = r.y; c = r.z;
        }
        float x = fmaf(u01(a), 2.0f, -1.0f);
        float y = fmaf(u01(b), 2.0f, -1.0f);
        float z = fmaf(u01(c), 2.0f, -1.0f);
        float l2 = x * x + y * y + z * z;
        if (l2 > 1e-4f && l2 <= 1.0f) {
            float inv = 1.0f / sqrtf(l2);
            dx = x * inv; dy = y * inv; dz = z * inv;
            return;
        }
    }
}

// FMath::VRandCone(n, 90 deg) (ARTS.cpp:313) or cosine-weighted (compat flag)
// (two halves: the sample in the cone's own frame depends on the two uniforms only — the cooperative walk lets idle lanes
// compute it for 64 bounces at a time — the turn into the world on the surface normal; sample_cone = one after the other)
__device__ __forceinline__ void cone_local(float U, float V, int cosine, float& lx, float& ly, float& cphi) {
    float sphi;
    if (cosine) {
        cphi = sqrtf(1.0f - V);
        sphi = sqrtf(V);
    } else {
        float x = fmaf(V, 2.0f, -1.0f);
        float r = sqrtf(fmaxf(0.0f, fmaf(-x, x, 1.0f)));
        if (x > 0.0f) { cphi = x; sphi = r; } else { cphi = r; sphi = -x; }
    }
    float st, ct;
    sincos2pi(U, st, ct);
    lx = sphi * ct; ly = sphi * st;
}
__device__ __forceinline__ void cone_world(float nx, float ny, float nz, float lx, float ly, float cphi, float& dx, float& dy, float& dz) {
    float sg = copysignf(1.0f, nz);
    float a = -1.0f / (sg + nz);
    float b = nx * ny * a;
    float t0 = fmaf(sg * nx * nx, a, 1.0f), t1 = sg * b, t2 = -sg * nx;
    float b0 = b, b1 = fmaf(ny * ny, a, sg), b2 = -ny;
    float d0 = fmaf(lx, t0, fmaf(ly, b0, cphi * nx));
    float d1 = fmaf(lx, t1, fmaf(ly, b1, cphi * ny));
    float d2 = fmaf(lx, t2, fmaf(ly, b2, cphi * nz));
    float l2 = d0 * d0 + d1 * d1 + d2 * d2;
    float inv = 1.0f / sqrtf(l2);
    dx = d0 * inv; dy = d1 * inv; dz = d2 * inv;
}
__device__ __forceinline__ void sample_cone(float nx, float ny, float nz, float U, float V, int cosine, float& dx,
                                            float& dy, float& dz) {
    float lx, ly, cphi;
    cone_local(U, V, cosine, lx, ly, cphi);
    cone_world(nx, ny, nz, lx, ly, cphi, dx, dy, dz);
}

// ---------------------------------------------------------------------------------------------------
// ray / triangle / box
// ---------------------------------------------------------------------------------------------------
struct Ray {
    float ox, oy, oz, dx, dy, dz;
    float ix, iy, iz;     // safe reciprocals for the slab test
    float nox, noy, noz;  // -o * inv: slab distances become one fma per plane
};

// Box tests only need to be conservative (boxes are padded far beyond this error), so the hardware
// reciprocal approximation is fine here; the triangle test uses IEEE division.
__device__ __forceinline__ float safe_rcp(float x) {
    if (fabsf(x) < 1e-20f) x = copysignf(1e-20f, x);
    return __builtin_amdgcn_rcpf(x);
}

__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    Ray r;
    r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx; r.dy = dy; r.dz = dz;
    r.ix = safe_rcp(dx); r.iy = safe_rcp(dy); r.iz = safe_rcp(dz);
    r.nox = -(ox * r.ix); r.noy = -(oy * r.iy); r.noz = -(oz * r.iz);
    return r;
}

// Moeller-Trumbore, two-sided, accepts t in (0, tmax].  Operation order is part of the spec.
__device__ __forceinline__ bool tri_hit(const float4 A, const float4 Bq, const float4 Cq, const Ray& r, float tmax,
                                        float& t_out) {
    const float v0x = A.x, v0y = A.y, v0z = A.z;
    const float e1x = A.w, e1y = Bq.x, e1z = Bq.y;
    const float e2x = Bq.z, e2y = Bq.w, e2z = Cq.x;
    float px = fmaf(r.dy, e2z, -(r.dz * e2y));
    float py = fmaf(r.dz, e2x, -(r.dx * e2z));
    float pz = fmaf(r.dx, e2y, -(r.dy * e2x));
    float det = fmaf(e1x, px, fmaf(e1y, py, e1z * pz));
    // barycentric tests on the un-normalised values, sign-normalised by det (exact: sign-bit xor).  All of
    // it is straight-line code behind ONE branch (bitwise &, no short-circuit exits: with a dozen lanes in
    // the test some lane nearly always needs every term, and each early exit costs exec-mask bookkeeping);
    // the one IEEE division is only paid by rays that are inside the triangle.
    const uint32_t sgn = __float_as_uint(det) & 0x80000000u;
    const float ad = fabsf(det);
    float sx = r.ox - v0x, sy = r.oy - v0y, sz = r.oz - v0z;
    float U = fmaf(sx, px, fmaf(sy, py, sz * pz));
    float us = __uint_as_float(__float_as_uint(U) ^ sgn);
    float qx = fmaf(sy, e1z, -(sz * e1y));
    float qy = fmaf(sz, e1x, -(sx * e1z));
    float qz = fmaf(sx, e1y, -(sy * e1x));
    float V = fmaf(r.dx, qx, fmaf(r.dy, qy, r.dz * qz));
    float vs = __uint_as_float(__float_as_uint(V) ^ sgn);
    float tn = fmaf(e2x, qx, fmaf(e2y, qy, e2z * qz));
    const bool inside = (det != 0.0f) & (us >= 0.0f) & (us <= ad) & (vs >= 0.0f) & ((us + vs) <= ad);
    if (!inside) return false;
    float t = tn / det;
    t_out = t;
    return (t > 0.0f) & (t <= tmax);
}


// one EvaluatePath segment term on E[b] (ARTS.cpp:381-398), in the reference's operation order
// LOBES: 0 / 1 = FS_FLAG_MATERIAL_LOBES known at compile time (the default connect kernel), -1 = read kp.lobes
// Band count of the connect kernels: a template constant for the counts in use (1, 4, 8: fully unrolled loops, the
// band energies stay in registers) or B = 0: kp.num_bands at run time (every other count: the same arithmetic, unrolled
// to FS_MAX_BANDS under a predicate).
template <int B> struct Bands { static constexpr int kMax = B ? B : FS_MAX_BANDS; };
template <int B> __device__ __forceinline__ int band_count(const KParams& kp) { return B ? B : kp.num_bands; }

template <int B, int LOBES = -1>
__device__ __forceinline__ void apply_segment(float (&E)[Bands<B>::kMax], float nd, uint32_t mat, float prob, const KParams& kp,
                                              const DeviceScene& sc) {
    const int NB = band_count<B>(kp);
    const bool lobes = LOBES < 0 ? kp.lobes != 0 : LOBES != 0;
    if (nd < kp.min_seg) return;  // ARTS.cpp:375-378
    float nd2 = nd * nd;
    float geo = 1.0f / (4 * kPi * nd2);            // ARTS.cpp:391
    float pw = powf(prob, kp.prob_exponent);       // ARTS.cpp:398
    // FS_FLAG_MATERIAL_LOBES (row f4): bits 16-17 of the record = lobe the walk took at this vertex (0 = diffuse,
    // also at a connection vertex); its gain replaces Absorption (the diffuse one still over pi)
    const uint32_t lobe = (lobes && mat != kNoMat) ? ((mat >> kLobeShift) & 3u) : 0u;
    if (lobes && mat != kNoMat) mat &= 0xFFFFu;
    bool has = (mat != kNoMat) && ((int32_t)mat < sc.num_materials);
    const float* coeff = lobes ? sc.lobe_gain + ((size_t)mat * 3 + lobe) * NB : sc.absorption + (size_t)mat * NB;
    const bool over_pi = !lobes || lobe == kLobeDiffuse;
#pragma unroll
    for (int b = 0; b < Bands<B>::kMax; ++b) {
        if (B == 0 && b >= NB) break;
        float bsdf = 1.0f;                                            // ARTS.cpp:382-386
        if (has) bsdf = over_pi ? coeff[b] / kPi : coeff[b];
        float e = E[b];
        e *= bsdf;
        e *= geo;
        e *= expf(-kp.air[b] * nd);                // ARTS.cpp:395-397
        e /= pw;
        E[b] = e;
    }
}

// The factors apply_segment multiplies in, computed apart from the running product: one lane per SEGMENT of a connected path
// evaluates them (the pow, the exponentials, the divisions), and the product over the path — strictly in the reference's
// order — is then four multiplications and a division per segment and band (connect_body, one pair per wave: a path of
// 160 segments took 40 us of one lane's time).  The same expressions as apply_segment, so the same bits.
template <int B>
struct SegFactors { float geo, pw; bool live; float bsdf[Bands<B>::kMax], ex[Bands<B>::kMax]; };
template <int B, int LOBES = -1>
__device__ __forceinline__ void segment_factors(SegFactors<B>& f, float nd, uint32_t mat, float prob, const KParams& kp, const DeviceScene& sc) {
    const int NB = band_count<B>(kp);
    const bool lobes = LOBES < 0 ? kp.lobes != 0 : LOBES != 0;
    f.live = !(nd < kp.min_seg);                   // ARTS.cpp:375-378
    float nd2 = nd * nd;
    f.geo = 1.0f / (4 * kPi * nd2);                // ARTS.cpp:391
    f.pw = powf(prob, kp.prob_exponent);           // ARTS.cpp:398
    const uint32_t lobe = (lobes && mat != kNoMat) ? ((mat >> kLobeShift) & 3u) : 0u;
    if (lobes && mat != kNoMat) mat &= 0xFFFFu;
    bool has = (mat != kNoMat) && ((int32_t)mat < sc.num_materials);
    const float* coeff = lobes ? sc.lobe_gain + ((size_t)mat * 3 + lobe) * NB : sc.absorption + (size_t)mat * NB;
    const bool over_pi = !lobes || lobe == kLobeDiffuse;
#pragma unroll
    for (int b = 0; b < Bands<B>::kMax; ++b) {
        f.bsdf[b] = 1.0f; f.ex[b] = 1.0f;
        if (B == 0 && b >= NB) continue;
        if (has) f.bsdf[b] = over_pi ? coeff[b] / kPi : coeff[b];      // ARTS.cpp:382-386
        f.ex[b] = expf(-kp.air[b] * nd);           // ARTS.cpp:395-397
    }
}

}  // namespace
}  // namespace fs
