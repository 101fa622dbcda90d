// fs_reflect.hip — fs_update_reflection_paths: the first-order specular reflections of every source of a tick.  The definitions
// (filter, leg 1, leg 2, the row) are those of include/frequensee.h, operation by operation; this file is their mapping onto the
// device, in two kernels.
//   reflect_scan_kernel: the scan scaffold of fs_dev_paths.hpp (scan_records) with this file's filter; a survivor's code is its leaf
// position.
//   reflect_confirm_kernel: one wave per source row, kBlock / 64 rows per workgroup as in direct_paths_kernel; the lanes stride over
// the row's candidates (at most FS_MAX_REFLECTION_CANDIDATES / 64 rounds).  A lane recomputes its candidate's D with the filter's
// own code, then runs leg 1 and leg 2 as chains (path_chain: the whole wave meets at every query, a lane without work idles along).
// The results wait in LDS by candidate slot; a confirmed one finds its rank by counting the smaller (length bits, input index) keys
// of its row, and ranks below max_paths store their path.  No sort network, no atomics.
//   Dynamic LDS of the confirm kernel: the stack rows [stack_rows][kBlock] | per wave kReflFields rows of max_candidates words.
#include "fs_dev_paths.hpp"

namespace fs {
namespace {

constexpr int kReflFields = 9;   // length bits | input index | material | P | d

// Step 1 of the rule for one (triangle record, source row); D is what the legs start from.
__device__ __forceinline__ bool reflect_filter(const TriEnds g, const float4 s4, const float (&L)[3], float m, float& Dx, float& Dy, float& Dz) {
    const bool side = (g.hS > 0.0f && g.hL > 0.0f) || (g.hS < 0.0f && g.hL < 0.0f);
    const float k = (2.0f * g.hS) / g.nn;
    const float Mx = s4.x - k * g.nx, My = s4.y - k * g.ny, Mz = s4.z - k * g.nz;   // S'
    Dx = Mx - L[0]; Dy = My - L[1]; Dz = Mz - L[2];
    const float px = Dy * g.e2z - Dz * g.e2y, py = Dz * g.e2x - Dx * g.e2z, pz = Dx * g.e2y - Dy * g.e2x;
    const float det = (g.e1x * px + g.e1y * py) + g.e1z * pz;
    const float inv = 1.0f / det;
    const float u = ((g.tx * px + g.ty * py) + g.tz * pz) * inv;
    const float qx = g.ty * g.e1z - g.tz * g.e1y, qy = g.tz * g.e1x - g.tx * g.e1z, qz = g.tx * g.e1y - g.ty * g.e1x;
    const float v = ((Dx * qx + Dy * qy) + Dz * qz) * inv;
    const float s = ((g.e2x * qx + g.e2y * qy) + g.e2z * qz) * inv;
    return !g.own && g.nn != 0.0f && side && det != 0.0f && u >= -m && v >= -m && (u + v) <= 1.0f + m && s > 0.0f && s < 1.0f;
}

__global__ __launch_bounds__(kBlock) void reflect_scan_kernel(DeviceScene sc, ReflectKParams rp) {
    scan_records(sc, rp.h, rp.counters, rp.cand, rp.max_candidates, [&](uint32_t leaf, const TriEnds g, const float4 s4, auto&& emit) {
        float Dx, Dy, Dz;
        if (reflect_filter(g, s4, rp.h.lis, rp.margin, Dx, Dy, Dz)) emit(leaf);
    });
}

__global__ __launch_bounds__(kBlock) void reflect_confirm_kernel(DeviceScene sc, ReflectKParams rp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] | per wave [kReflFields][max_candidates]
    int* stack = &s_dyn[threadIdx.x];
    const ConfirmRow cr = confirm_row(rp.h, rp.counters, rp.cand, rp.max_candidates);
    const int lane = cr.lane, n = cr.n, row = cr.row;
    const float4 s4 = cr.s4;
    const int maxc = rp.max_candidates, B = rp.h.num_bands;
    uint32_t* w = reinterpret_cast<uint32_t*>(s_dyn + (size_t)sc.stack_rows * kBlock) + (size_t)cr.wave * kReflFields * maxc;
    uint32_t found = 0u;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {   // (wave-uniform)
        const int c = base + lane;
        const bool mine = c < n;
        const int leaf = mine ? (int)cr.list[c] : 0;
        const Tri48 rec = sc.tris[leaf];
        float Dx, Dy, Dz;
        (void)reflect_filter(tri_ends(rec, s4, rp.h), s4, rp.h.lis, rp.margin, Dx, Dy, Dz);
        const float len1 = sqrtf((Dx * Dx + Dy * Dy) + Dz * Dz);
        const float inv1 = 1.0f / len1;
        const float dx = Dx * inv1, dy = Dy * inv1, dz = Dz * inv1;
        // leg 1 ends at the first triangle that is not an own actor's, and asks that it be the candidate's record: t = the distance
        // from the leg's start, P = the hit point
        AskLeaf l1{leaf};
        (void)path_chain(sc, rp.h, cr.src_object, mine, rp.h.lis[0], rp.h.lis[1], rp.h.lis[2], dx, dy, dz, len1, stack, l1);
        const float Px = l1.Px, Py = l1.Py, Pz = l1.Pz;
        const float ex = s4.x - Px, ey = s4.y - Py, ez = s4.z - Pz;
        const float len2 = sqrtf((ex * ex + ey * ey) + ez * ez);
        const bool second = mine && l1.hit && len2 != 0.0f;
        const float inv2 = 1.0f / (second ? len2 : 1.0f);
        const float d2x = ex * inv2, d2y = ey * inv2, d2z = ez * inv2;
        // leg 2 is chain(o, d, len) with max_surfaces = 0 and asks for reached (with crossed == 0)
        const bool ok = path_chain(sc, rp.h, cr.src_object, second, fmaf(rp.offset, d2x, Px), fmaf(rp.offset, d2y, Py), fmaf(rp.offset, d2z, Pz),
                                   d2x, d2y, d2z, (len2 - rp.offset) - rp.h.pullback, stack, StopAtHit()) == kChainReached;
        const float length = l1.t + len2;
        if (mine) {
            w[0 * maxc + c] = ok ? __float_as_uint(length) : 0xFFFFFFFFu;
            w[1 * maxc + c] = ok ? __float_as_uint(rec.c.z) : 0xFFFFFFFFu;
            w[2 * maxc + c] = __float_as_uint(rec.c.y);
            w[3 * maxc + c] = __float_as_uint(Px); w[4 * maxc + c] = __float_as_uint(Py); w[5 * maxc + c] = __float_as_uint(Pz);
            w[6 * maxc + c] = __float_as_uint(dx); w[7 * maxc + c] = __float_as_uint(dy); w[8 * maxc + c] = __float_as_uint(dz);
        }
        found += (uint32_t)__popcll(__ballot(ok));
    }
    __syncthreads();
    if (!cr.row_ok) return;
    const uint32_t returned = min(found, (uint32_t)rp.max_paths);
    fs_reflection_path* out = rp.paths + (size_t)row * rp.max_paths;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {
        const int c = base + lane;
        if (c >= n || w[c] == 0xFFFFFFFFu) continue;   // (not confirmed: both key words all ones, kNoPathKey)
        const uint32_t rank = rank_among((uint32_t)n, path_key(w[c], w[maxc + c]), [&](uint32_t j) { return path_key(w[j], w[maxc + j]); });
        if (rank >= (uint32_t)rp.max_paths) continue;
        fs_reflection_path* o = out + rank;
        const float length = __uint_as_float(w[c]);
        const uint32_t mat = w[2 * maxc + c];
        o->length = length;
        o->delay = path_delay(rp.h, length);
        o->point[0] = __uint_as_float(w[3 * maxc + c]); o->point[1] = __uint_as_float(w[4 * maxc + c]); o->point[2] = __uint_as_float(w[5 * maxc + c]);
        o->direction[0] = __uint_as_float(w[6 * maxc + c]); o->direction[1] = __uint_as_float(w[7 * maxc + c]); o->direction[2] = __uint_as_float(w[8 * maxc + c]);
        o->triangle = w[maxc + c];
        o->material = mat;
        const float* g = specular_gain(sc, mat, B);
#pragma unroll
        for (int b = 0; b < FS_MAX_BANDS; ++b) o->reflectance[b] = b < B ? (g != nullptr ? g[b] : 1.0f) : 0.0f;
    }
    zero_tail(out, lane, returned, rp.max_paths);
    if (lane == 0) {
        fs_reflection_row* r = rp.rows + row;
        r->candidates = cr.cands;
        r->found = found;
        r->returned = returned;
        r->flags = cr.overflow ? FS_REFLECTION_OVERFLOW : 0u;
    }
}

}  // namespace

void launch_reflection_paths(const DeviceScene& sc, const ReflectKParams& rp, hipStream_t s) {
    const size_t slots = sizeof(uint32_t) * (size_t)kRowsPerBlock * kReflFields * (size_t)rp.max_candidates;   // the results, by candidate
    launch_scan_confirm(reflect_scan_kernel, reflect_confirm_kernel, sc, rp, slots, s);
}

}  // namespace fs
