// fs_reflect2.hip — fs_update_reflection2_paths: the second-order specular reflections of every source of a tick.  The definitions
// (near set, pair filter, the three legs, the row) are those of include/frequensee.h, operation by operation; this file is their
// mapping onto the device, in three kernels.
//   reflect2_near_kernel: the scan scaffold of fs_dev_paths.hpp (scan_records) with step 0 as its filter; a near triangle's code is
// its leaf position, the row's near list the "candidate list" of the scaffold.
//   reflect2_pair_kernel: the hot one — the pair scaffold (pair_records).  The held entry is a near triangle in the role of a (what
// MT(L, D, a) needs of it that does not depend on b — tv, q, e2.q — included), the streamed one a near triangle in the role of b:
// hS, S1, n_b and the record, 16 words.  The strict-side test (h1 against hL) comes before any divide — it rejects a sixth of the
// pairs in a closed shoebox — and the rest ends at MT(L, D, a) but for a handful.
//   reflect2_confirm_kernel: one wave per source row (confirm_row), the lanes stride over the row's candidates (at most
// FS_MAX_REFLECTION2_CANDIDATES / 64 = 16 rounds).  A lane recomputes S1 and D with the pair filter's own code — the same bits — and
// runs the three legs as chains (path_chain) one after the other; a lane whose candidate has already failed idles along.  A
// confirmed one takes the next place of the row's list in the call's device staging (compact_slot), written and read by the row's
// own wave only; the rank is counted over that list by the 96-bit key (length bits, a, b).  Plain vector stores, no sort network.
//   Dynamic LDS of the confirm kernel: the stack rows [stack_rows][kBlock], nothing else.
#include "fs_dev_paths.hpp"

namespace fs {
namespace {

// what the pair filter reads of triangle a: nothing of it depends on b or on S
struct PairA {
    float v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z;
    float nx, ny, nz, nn, hL;
    float tx, ty, tz;      // tv = L - v0
    float qx, qy, qz, e2q; // q = cross(tv, e1), e2.q
};
__device__ __forceinline__ PairA pair_a(const TriEnds g) {
    PairA a;
    a.v0x = g.v0x; a.v0y = g.v0y; a.v0z = g.v0z; a.e1x = g.e1x; a.e1y = g.e1y; a.e1z = g.e1z; a.e2x = g.e2x; a.e2y = g.e2y; a.e2z = g.e2z;
    a.nx = g.nx; a.ny = g.ny; a.nz = g.nz; a.nn = g.nn; a.hL = g.hL;
    a.tx = g.tx; a.ty = g.ty; a.tz = g.tz;
    a.qx = g.ty * g.e1z - g.tz * g.e1y; a.qy = g.tz * g.e1x - g.tx * g.e1z; a.qz = g.tx * g.e1y - g.ty * g.e1x;
    a.e2q = (g.e2x * a.qx + g.e2y * a.qy) + g.e2z * a.qz;
    return a;
}

// what the pair filter reads of triangle b and the source: the image S1 of S in b, hS, the normal and the record — 16 words
struct PairB {
    float S1x, S1y, S1z, hS;
    float nx, ny, nz, v0x;
    float v0y, v0z, e1x, e1y;
    float e1z, e2x, e2y, e2z;
};
__device__ __forceinline__ PairB pair_b(const TriEnds g, const float4 s4) {
    PairB b;
    const float k1 = (2.0f * g.hS) / g.nn;
    b.S1x = s4.x - k1 * g.nx; b.S1y = s4.y - k1 * g.ny; b.S1z = s4.z - k1 * g.nz;
    b.hS = g.hS;
    b.nx = g.nx; b.ny = g.ny; b.nz = g.nz;
    b.v0x = g.v0x; b.v0y = g.v0y; b.v0z = g.v0z; b.e1x = g.e1x; b.e1y = g.e1y; b.e1z = g.e1z; b.e2x = g.e2x; b.e2y = g.e2y; b.e2z = g.e2z;
    return b;
}

// Step 0 of the rule for one (triangle record, source row)
__device__ __forceinline__ bool reflect2_near(const TriEnds g, const float4 s4, float max_length) {
    const float ax = s4.x - g.v0x, ay = s4.y - g.v0y, az = s4.z - g.v0z;
    const float la = sqrtf((ax * ax + ay * ay) + az * az);
    const float lb = sqrtf((g.tx * g.tx + g.ty * g.ty) + g.tz * g.tz);
    const float reach = fmaxf(sqrtf((g.e1x * g.e1x + g.e1y * g.e1y) + g.e1z * g.e1z), sqrtf((g.e2x * g.e2x + g.e2y * g.e2y) + g.e2z * g.e2z));
    return !g.own && g.nn != 0.0f && ((la + lb) - (reach + reach)) <= max_length;
}

// Step 1 of the rule for one ordered pair (b, a) of near triangles; D is what the legs start from.  The early returns change no bit:
// every operation is rounded on its own wherever it stands.
__device__ __forceinline__ bool pair_filter(const PairA& a, const PairB& b, const float (&L)[3], float m, float max_length, float& Dx, float& Dy,
                                            float& Dz) {
    const float rx = b.S1x - a.v0x, ry = b.S1y - a.v0y, rz = b.S1z - a.v0z;
    const float h1 = (rx * a.nx + ry * a.ny) + rz * a.nz;
    if (!((h1 > 0.0f && a.hL > 0.0f) || (h1 < 0.0f && a.hL < 0.0f))) return false;
    const float k2 = (2.0f * h1) / a.nn;
    Dx = (b.S1x - k2 * a.nx) - L[0]; Dy = (b.S1y - k2 * a.ny) - L[1]; Dz = (b.S1z - k2 * a.nz) - L[2];
    // MT(L, D, a)
    const float px = Dy * a.e2z - Dz * a.e2y, py = Dz * a.e2x - Dx * a.e2z, pz = Dx * a.e2y - Dy * a.e2x;
    const float det = (a.e1x * px + a.e1y * py) + a.e1z * pz;
    const float inv = 1.0f / det;
    const float u = ((a.tx * px + a.ty * py) + a.tz * pz) * inv;
    const float v = ((Dx * a.qx + Dy * a.qy) + Dz * a.qz) * inv;
    const float s = a.e2q * inv;
    const float len = sqrtf((Dx * Dx + Dy * Dy) + Dz * Dz);
    if (!(b.hS != 0.0f && det != 0.0f && u >= -m && v >= -m && (u + v) <= 1.0f + m && s > 0.0f && s < 1.0f && len <= max_length)) return false;
    const float Qx = fmaf(s, Dx, L[0]), Qy = fmaf(s, Dy, L[1]), Qz = fmaf(s, Dz, L[2]);
    const float wx = Qx - b.v0x, wy = Qy - b.v0y, wz = Qz - b.v0z;   // tv of MT(Q, D2, b)
    const float hQ = (wx * b.nx + wy * b.ny) + wz * b.nz;
    if (!((hQ > 0.0f && b.hS > 0.0f) || (hQ < 0.0f && b.hS < 0.0f))) return false;
    // MT(Q, D2, b)
    const float Ex = b.S1x - Qx, Ey = b.S1y - Qy, Ez = b.S1z - Qz;
    const float p2x = Ey * b.e2z - Ez * b.e2y, p2y = Ez * b.e2x - Ex * b.e2z, p2z = Ex * b.e2y - Ey * b.e2x;
    const float det2 = (b.e1x * p2x + b.e1y * p2y) + b.e1z * p2z;
    const float inv2 = 1.0f / det2;
    const float u2 = ((wx * p2x + wy * p2y) + wz * p2z) * inv2;
    const float q2x = wy * b.e1z - wz * b.e1y, q2y = wz * b.e1x - wx * b.e1z, q2z = wx * b.e1y - wy * b.e1x;
    const float v2 = ((Ex * q2x + Ey * q2y) + Ez * q2z) * inv2;
    const float s2 = ((b.e2x * q2x + b.e2y * q2y) + b.e2z * q2z) * inv2;
    return det2 != 0.0f && u2 >= -m && v2 >= -m && (u2 + v2) <= 1.0f + m && s2 > 0.0f && s2 < 1.0f;
}

__global__ __launch_bounds__(kBlock) void reflect2_near_kernel(DeviceScene sc, Reflect2KParams rp) {
    scan_records(sc, rp.h, rp.l.near_counters, rp.l.near, rp.l.max_near, [&](uint32_t leaf, const TriEnds g, const float4 s4, auto&& emit) {
        if (reflect2_near(g, s4, rp.max_length)) emit(leaf);
    });
}

__global__ __launch_bounds__(kBlock) void reflect2_pair_kernel(DeviceScene sc, Reflect2KParams rp) {
    pair_records(
        rp.h, rp.l, [&](uint32_t leaf, const float4 s4) { return pair_a(tri_ends(sc.tris[leaf], s4, rp.h)); },
        [&](uint32_t leaf, const float4 s4) {
            const PairB b = pair_b(tri_ends(sc.tris[leaf], s4, rp.h), s4);
            return PairRow{make_float4(b.S1x, b.S1y, b.S1z, b.hS), make_float4(b.nx, b.ny, b.nz, b.v0x), make_float4(b.v0y, b.v0z, b.e1x, b.e1y),
                           make_float4(b.e1z, b.e2x, b.e2y, b.e2z)};
        },
        [&](const PairA& a, const PairRow r, const float4) {
            const PairB b = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w, r.d.x, r.d.y, r.d.z, r.d.w};
            float Dx, Dy, Dz;
            return pair_filter(a, b, rp.h.lis, rp.margin, rp.max_length, Dx, Dy, Dz);
        });
}

__global__ __launch_bounds__(kBlock) void reflect2_confirm_kernel(DeviceScene sc, Reflect2KParams rp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock]
    int* stack = &s_dyn[threadIdx.x];
    const ConfirmRow cr = confirm_row(rp.h, rp.l);
    const int lane = cr.lane, n = cr.n, row = cr.row, B = rp.h.num_bands;
    const float4 s4 = cr.s4;
    const uint32_t near = near_count(cr, rp.l);
    const uint32_t* list = rp.l.near + (size_t)cr.slot * rp.l.max_near;
    Reflect2Record* conf = rp.conf + (size_t)cr.slot * rp.l.max_candidates;
    uint32_t found = 0u;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {   // (wave-uniform; n > 0 only where the near list is whole and has two entries at least)
        const int c = base + lane;
        const bool mine = c < n;
        const uint32_t code = mine ? cr.list[c] : 0u;
        const int leafA = (int)pair_held(list, code), leafB = (int)pair_streamed(list, code);
        const Tri48 recA = sc.tris[leafA], recB = sc.tris[leafB];
        const PairB pb = pair_b(tri_ends(recB, s4, rp.h), s4);
        float Dx = 1.0f, Dy = 0.0f, Dz = 0.0f;
        (void)pair_filter(pair_a(tri_ends(recA, s4, rp.h)), pb, rp.h.lis, rp.margin, rp.max_length, Dx, Dy, Dz);
        const float len1 = sqrtf((Dx * Dx + Dy * Dy) + Dz * Dz);
        const float inv1 = 1.0f / len1;
        const float dx = Dx * inv1, dy = Dy * inv1, dz = Dz * inv1;
        // leg 1 ends at the first triangle that is not an own actor's, and asks that it be a
        AskLeaf la{leafA};
        (void)path_chain(sc, rp.h, cr.src_object, mine, rp.h.lis[0], rp.h.lis[1], rp.h.lis[2], dx, dy, dz, len1, stack, la);
        // leg 2, from PA towards the image S1, asks for b
        const float Ex = pb.S1x - la.Px, Ey = pb.S1y - la.Py, Ez = pb.S1z - la.Pz;
        const float len2 = sqrtf((Ex * Ex + Ey * Ey) + Ez * Ez);
        const bool second = mine && la.hit && len2 != 0.0f;
        const float inv2 = 1.0f / (second ? len2 : 1.0f);
        const float d2x = Ex * inv2, d2y = Ey * inv2, d2z = Ez * inv2;
        AskLeaf lb{leafB};
        (void)path_chain(sc, rp.h, cr.src_object, second, fmaf(rp.offset, d2x, la.Px), fmaf(rp.offset, d2y, la.Py), fmaf(rp.offset, d2z, la.Pz), d2x,
                         d2y, d2z, len2 - rp.offset, stack, lb);
        // leg 3 is chain(o, d, len) with max_surfaces = 0 and asks for reached (with crossed == 0)
        const float ex = s4.x - lb.Px, ey = s4.y - lb.Py, ez = s4.z - lb.Pz;
        const float len3 = sqrtf((ex * ex + ey * ey) + ez * ez);
        const bool third = second && lb.hit && len3 != 0.0f;
        const float inv3 = 1.0f / (third ? len3 : 1.0f);
        const float d3x = ex * inv3, d3y = ey * inv3, d3z = ez * inv3;
        const bool ok = path_chain(sc, rp.h, cr.src_object, third, fmaf(rp.offset, d3x, lb.Px), fmaf(rp.offset, d3y, lb.Py), fmaf(rp.offset, d3z, lb.Pz),
                                   d3x, d3y, d3z, (len3 - rp.offset) - rp.h.pullback, stack, StopAtHit()) == kChainReached;
        const unsigned long long votes = __ballot(ok);
        if (ok) {
            Reflect2Record* o = conf + found + compact_slot(votes, lane);
            o->length_bits = __float_as_uint((la.t + (rp.offset + lb.t)) + len3);
            o->a = __float_as_uint(recA.c.z); o->b = __float_as_uint(recB.c.z);
            o->pa[0] = la.Px; o->pa[1] = la.Py; o->pa[2] = la.Pz;
            o->pb[0] = lb.Px; o->pb[1] = lb.Py; o->pb[2] = lb.Pz;
            o->direction[0] = dx; o->direction[1] = dy; o->direction[2] = dz;
            o->material[0] = __float_as_uint(recA.c.y); o->material[1] = __float_as_uint(recB.c.y);
        }
        found += (uint32_t)__popcll(votes);
    }
    __syncthreads();   // the list is in memory for every lane of the wave that wrote it
    if (!cr.row_ok) return;
    const uint32_t returned = min(found, (uint32_t)rp.max_paths);
    fs_reflection2_path* out = rp.paths + (size_t)row * rp.max_paths;
#pragma unroll 1
    for (uint32_t base = 0u; base < found; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        if (e >= found) continue;
        const Reflect2Record me = conf[e];
        const uint32_t rank = rank_among(found, PathKey96{path_key(me.length_bits, me.a), me.b}, [&](uint32_t j) {
            const Reflect2Record* x = conf + j;
            return PathKey96{path_key(x->length_bits, x->a), x->b};
        });
        if (rank >= (uint32_t)rp.max_paths) continue;
        fs_reflection2_path* o = out + rank;
        const float length = __uint_as_float(me.length_bits);
        o->length = length;
        o->delay = path_delay(rp.h, length);
        o->point[0][0] = me.pa[0]; o->point[0][1] = me.pa[1]; o->point[0][2] = me.pa[2];
        o->point[1][0] = me.pb[0]; o->point[1][1] = me.pb[1]; o->point[1][2] = me.pb[2];
        o->direction[0] = me.direction[0]; o->direction[1] = me.direction[1]; o->direction[2] = me.direction[2];
        o->triangle[0] = me.a; o->triangle[1] = me.b;
        o->material[0] = me.material[0]; o->material[1] = me.material[1];
        const float *gA = specular_gain(sc, me.material[0], B), *gB = specular_gain(sc, me.material[1], B);
#pragma unroll
        for (int b = 0; b < FS_MAX_BANDS; ++b) o->reflectance[b] = b < B ? (gA != nullptr ? gA[b] : 1.0f) * (gB != nullptr ? gB[b] : 1.0f) : 0.0f;
    }
    zero_tail(out, lane, returned, rp.max_paths);
    if (lane == 0) {
        fs_reflection2_row* r = rp.rows + row;
        r->near = near;
        r->candidates = cr.cands;
        r->found = found;
        r->returned = returned;
        r->flags = pair_row_flags(cr, rp.l, near, FS_REFLECTION2_NEAR_OVERFLOW, FS_REFLECTION2_OVERFLOW);
    }
}

}  // namespace

void launch_reflection2_paths(const DeviceScene& sc, const Reflect2KParams& rp, hipStream_t s) {
    launch_near_pair_confirm(reflect2_near_kernel, reflect2_pair_kernel, reflect2_confirm_kernel, sc, rp, 1, rp.l.max_near, 0, s);   // a triangle: one near entry
}

}  // namespace fs
