// fs_mixed.hip — fs_update_mixed_paths: the paths of every source of a tick that reflect off one triangle and bend round one edge,
// what is left of the early reflections of a source behind a partition.  The definitions (near set, filter, the four legs, the merge,
// the row) are those of include/frequensee.h, operation by operation; this file is their mapping onto the device, in three kernels on
// the scaffolds of fs_dev_paths.hpp.
//   mixed_near_kernel: the scan scaffold (scan_records) with step 0 as its filter.  A record contributes up to four entries to the
// row's one near list: its three edge records (code = leaf position * 4 + edge) and itself as a face (leaf position * 4 + 3).
//   mixed_pair_kernel: the hot one — the pair scaffold (pair_records) over a list of two kinds.  The held entry is an edge record
// (a, w, ww, n, v0, o: 16 words that depend on neither the face nor the end); a thread that holds a face has nothing to test.  The
// streamed entry is a face: the record and the two images of it, L' for end 0 and S' for end 1, 15 words, and a tag — its leaf
// position and which ends it can serve.  The tag is the same in every lane (an LDS broadcast), so a streamed edge record costs the
// wave one branch.  The test runs the first-order diffraction filter on the unfolded ends and then MT(E, A' - E, m) for both ends and
// answers with the mask of the ends that passed (for_each_verdict); the strict-side test stands before any divide.
//   mixed_confirm_kernel: one wave per source row (confirm_row), the lanes stride over the row's candidates (at most
// FS_MAX_MIXED_CANDIDATES / 64 = 32 rounds).  A lane recomputes its candidate's values with the filter's own code — the same bits —
// and runs the four legs, the short one first, as chains (path_chain) round one copy of the traversal; leg 3 asks for the reflector
// (AskLeaf) and hands its hit point to leg 4.  A confirmed one takes the next place of the row's list in the call's device staging
// (compact_slot), written and read by the row's own wave only; merge (mark_kept) and rank are counted over that list by the 96-bit
// key (length bits, end and m, 4 i + j).  Plain vector stores, no sort network.
//   Dynamic LDS of the confirm kernel: the stack rows [stack_rows][kBlock], nothing else.
#include "fs_dev_paths.hpp"

namespace fs {
namespace {

constexpr uint32_t kFaceCode = 3u;        // the "edge" of a near-list code that stands for the triangle itself
constexpr uint32_t kNotAnEdge = ~0u;      // MixedEdge::leaf of a held entry that is a face

// Step 0 for one (triangle record, source row): the face by the second-order reflection rule, an edge record by the same bound
// with the origin at its start
__device__ __forceinline__ bool mixed_near_face(const TriEnds g, const float4 s4, float max_length) {
    const float ax = s4.x - g.v0x, ay = s4.y - g.v0y, az = s4.z - g.v0z;
    const float la = sqrtf((ax * ax + ay * ay) + az * az);
    const float lb = sqrtf((g.tx * g.tx + g.ty * g.ty) + g.tz * g.tz);
    const float reach = fmaxf(sqrtf((g.e1x * g.e1x + g.e1y * g.e1y) + g.e1z * g.e1z), sqrtf((g.e2x * g.e2x + g.e2y * g.e2y) + g.e2z * g.e2z));
    return !g.own && g.nn != 0.0f && ((la + lb) - (reach + reach)) <= max_length;
}
__device__ __forceinline__ bool mixed_near_edge(const TriEnds g, const EdgeRec e, const float4 s4, const float (&L)[3], float max_length) {
    const float rSx = s4.x - e.ax, rSy = s4.y - e.ay, rSz = s4.z - e.az;
    const float rLx = L[0] - e.ax, rLy = L[1] - e.ay, rLz = L[2] - e.az;
    const float la = sqrtf((rSx * rSx + rSy * rSy) + rSz * rSz);
    const float lb = sqrtf((rLx * rLx + rLy * rLy) + rLz * rLz);
    const float reach = sqrtf(e.ww);
    return !g.own && g.nn != 0.0f && e.ww != 0.0f && e.oo != 0.0f && ((la + lb) - (reach + reach)) <= max_length;
}

// what the filter reads of the edge record r: nothing of it depends on the face or the end
struct MixedEdge {
    float ax, ay, az, wx, wy, wz, ww;
    float nx, ny, nz, v0x, v0y, v0z;
    float ox, oy, oz;
    uint32_t leaf;   // the leaf position of its triangle, kNotAnEdge for a held face
};
__device__ __forceinline__ MixedEdge mixed_edge(const TriEnds g, const EdgeRec e, uint32_t leaf) {
    MixedEdge x;
    x.ax = e.ax; x.ay = e.ay; x.az = e.az; x.wx = e.wx; x.wy = e.wy; x.wz = e.wz; x.ww = e.ww;
    x.nx = g.nx; x.ny = g.ny; x.nz = g.nz; x.v0x = g.v0x; x.v0y = g.v0y; x.v0z = g.v0z;
    x.ox = e.ox; x.oy = e.oy; x.oz = e.oz;
    x.leaf = leaf;
    return x;
}

// what the filter reads of the face m: the images A' of both ends, the record, and tag = leaf position << 2 | the ends whose hA != 0
// (bit 0: end 0, the image of L; bit 1: end 1, the image of S) — 16 words
struct MixedFace {
    float L1x, L1y, L1z, S1x;
    float S1y, S1z, v0x, v0y;
    float v0z, e1x, e1y, e1z;
    float e2x, e2y, e2z;
    uint32_t tag;
};
__device__ __forceinline__ MixedFace mixed_face(const TriEnds g, const float4 s4, const float (&L)[3], uint32_t leaf) {
    MixedFace f;
    const float kL = (2.0f * g.hL) / g.nn, kS = (2.0f * g.hS) / g.nn;
    f.L1x = L[0] - kL * g.nx; f.L1y = L[1] - kL * g.ny; f.L1z = L[2] - kL * g.nz;
    f.S1x = s4.x - kS * g.nx; f.S1y = s4.y - kS * g.ny; f.S1z = s4.z - kS * g.nz;
    f.v0x = g.v0x; f.v0y = g.v0y; f.v0z = g.v0z; f.e1x = g.e1x; f.e1y = g.e1y; f.e1z = g.e1z; f.e2x = g.e2x; f.e2y = g.e2y; f.e2z = g.e2z;
    f.tag = (leaf << 2) | (g.hL != 0.0f ? 1u : 0u) | (g.hS != 0.0f ? 2u : 0u);
    return f;
}

// what step 1 hands on to the legs and the row
struct MixedCandidate {
    float Ex, Ey, Ez;       // the apex
    float A1x, A1y, A1z;    // A', the image of the end next to the reflector
    float ux, uy, uz, lS;   // u = S - E of the substituted ends
    float vx, vy, vz, lL;   // v = E - L
    float length, bend;
    float hZ;               // the plane distance of Z from the edge's triangle
};

// Step 1 of the rule for one (edge record, face, end).  The early returns change no bit: every operation is rounded on its own
// wherever it stands.
__device__ __forceinline__ bool mixed_filter(const MixedEdge& e, const MixedFace& f, int end, const float4 s4, const float (&L)[3], float m,
                                             float max_detour, float max_length, MixedCandidate& c) {
    // the ends of the first-order diffraction rule: A' stands in for S (end 1) or for L (end 0)
    const float Sx = end ? f.S1x : s4.x, Sy = end ? f.S1y : s4.y, Sz = end ? f.S1z : s4.z;
    const float Lx = end ? L[0] : f.L1x, Ly = end ? L[1] : f.L1y, Lz = end ? L[2] : f.L1z;
    const float sx = Sx - e.v0x, sy = Sy - e.v0y, sz = Sz - e.v0z;
    const float hS = (sx * e.nx + sy * e.ny) + sz * e.nz;
    const float lx = Lx - e.v0x, ly = Ly - e.v0y, lz = Lz - e.v0z;
    const float hL = (lx * e.nx + ly * e.ny) + lz * e.nz;
    if (!((hS > 0.0f && hL < 0.0f) || (hS < 0.0f && hL > 0.0f))) return false;
    const float rSx = Sx - e.ax, rSy = Sy - e.ay, rSz = Sz - e.az;
    const float rLx = Lx - e.ax, rLy = Ly - e.ay, rLz = Lz - e.az;
    const float tS = ((rSx * e.wx + rSy * e.wy) + rSz * e.wz) / e.ww;
    const float tL = ((rLx * e.wx + rLy * e.wy) + rLz * e.wz) / e.ww;
    const float cSx = rSy * e.wz - rSz * e.wy, cSy = rSz * e.wx - rSx * e.wz, cSz = rSx * e.wy - rSy * e.wx;
    const float cLx = rLy * e.wz - rLz * e.wy, cLy = rLz * e.wx - rLx * e.wz, cLz = rLx * e.wy - rLy * e.wx;
    const float dS = sqrtf(((cSx * cSx + cSy * cSy) + cSz * cSz) / e.ww);
    const float dL = sqrtf(((cLx * cLx + cLy * cLy) + cLz * cLz) / e.ww);
    const float sum = dS + dL;
    const float t = tS + ((tL - tS) * dS) / sum;
    if (!(sum != 0.0f && t >= -m && t <= 1.0f + m)) return false;
    const float Ex = fmaf(t, e.wx, e.ax), Ey = fmaf(t, e.wy, e.ay), Ez = fmaf(t, e.wz, e.az);
    const float ux = Sx - Ex, uy = Sy - Ey, uz = Sz - Ez;
    const float vx = Ex - Lx, vy = Ey - Ly, vz = Ez - Lz;
    const float lS = sqrtf((ux * ux + uy * uy) + uz * uz);
    const float lL = sqrtf((vx * vx + vy * vy) + vz * vz);
    const float length = lS + lL;
    const float gx = Sx - Lx, gy = Sy - Ly, gz = Sz - Lz;
    const float unfolded = sqrtf((gx * gx + gy * gy) + gz * gz);
    const float bend = length - unfolded;
    const float s = hS / (hS - hL);
    const float Xx = fmaf(s, Lx - Sx, Sx), Xy = fmaf(s, Ly - Sy, Sy), Xz = fmaf(s, Lz - Sz, Sz);
    const float qx = Xx - Ex, qy = Xy - Ey, qz = Xz - Ez;
    const float shadow = (qx * e.ox + qy * e.oy) + qz * e.oz;
    c.Ex = Ex; c.Ey = Ey; c.Ez = Ez;
    c.A1x = end ? Sx : Lx; c.A1y = end ? Sy : Ly; c.A1z = end ? Sz : Lz;
    c.ux = ux; c.uy = uy; c.uz = uz; c.lS = lS;
    c.vx = vx; c.vy = vy; c.vz = vz; c.lL = lL;
    c.length = length; c.bend = bend;
    c.hZ = end ? hL : hS;
    if (!(lS != 0.0f && lL != 0.0f && bend <= max_detour && length <= max_length && shadow <= 0.0f)) return false;
    // MT(E, D, m) with D = A' - E
    const float Dx = c.A1x - Ex, Dy = c.A1y - Ey, Dz = c.A1z - Ez;
    const float px = Dy * f.e2z - Dz * f.e2y, py = Dz * f.e2x - Dx * f.e2z, pz = Dx * f.e2y - Dy * f.e2x;
    const float det = (f.e1x * px + f.e1y * py) + f.e1z * pz;
    const float inv = 1.0f / det;
    const float tx = Ex - f.v0x, ty = Ey - f.v0y, tz = Ez - f.v0z;
    const float bu = ((tx * px + ty * py) + tz * pz) * inv;
    const float kx = ty * f.e1z - tz * f.e1y, ky = tz * f.e1x - tx * f.e1z, kz = tx * f.e1y - ty * f.e1x;
    const float bv = ((Dx * kx + Dy * ky) + Dz * kz) * inv;
    const float bs = ((f.e2x * kx + f.e2y * ky) + f.e2z * kz) * inv;
    return det != 0.0f && bu >= -m && bv >= -m && (bu + bv) <= 1.0f + m && bs > 0.0f && bs < 1.0f;
}

__global__ __launch_bounds__(kBlock) void mixed_near_kernel(DeviceScene sc, MixedKParams mp) {
    scan_records(sc, mp.h, mp.l.near_counters, mp.l.near, mp.l.max_near, [&](uint32_t leaf, const TriEnds g, const float4 s4, auto&& emit) {
#pragma unroll
        for (int edge = 0; edge < 3; ++edge)
            if (mixed_near_edge(g, edge_rec(g, edge), s4, mp.h.lis, mp.max_length)) emit(leaf * 4u + (uint32_t)edge);
        if (mixed_near_face(g, s4, mp.max_length)) emit(leaf * 4u + kFaceCode);
    });
}

__global__ __launch_bounds__(kBlock) void mixed_pair_kernel(DeviceScene sc, MixedKParams mp) {
    pair_records(
        mp.h, mp.l,
        [&](uint32_t code, const float4 s4) {
            const TriEnds g = tri_ends(sc.tris[code >> 2], s4, mp.h);
            const uint32_t edge = code & 3u;
            return mixed_edge(g, edge_rec(g, (int)edge), edge == kFaceCode ? kNotAnEdge : code >> 2);
        },
        [&](uint32_t code, const float4 s4) {
            const TriEnds g = tri_ends(sc.tris[code >> 2], s4, mp.h);
            MixedFace f = mixed_face(g, s4, mp.h.lis, code >> 2);
            if ((code & 3u) != kFaceCode) f.tag = 0u;   // an edge record in the streamed role: no end to serve
            return PairRow{make_float4(f.L1x, f.L1y, f.L1z, f.S1x), make_float4(f.S1y, f.S1z, f.v0x, f.v0y), make_float4(f.v0z, f.e1x, f.e1y, f.e1z),
                           make_float4(f.e2x, f.e2y, f.e2z, __uint_as_float(f.tag))};
        },
        [&](const MixedEdge& e, const PairRow r, const float4 s4) {
            const uint32_t tag = __float_as_uint(r.d.w);
            if ((tag & 3u) == 0u || e.leaf == kNotAnEdge || e.leaf == tag >> 2) return 0u;   // (the first: the same in every lane)
            const MixedFace f = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w, r.d.x, r.d.y, r.d.z, tag};
            uint32_t mask = 0u;
#pragma unroll
            for (int end = 0; end < 2; ++end) {
                MixedCandidate c;
                if ((tag >> end & 1u) != 0u && mixed_filter(e, f, end, s4, mp.h.lis, mp.margin, mp.max_detour, mp.max_length, c)) mask |= 1u << end;
            }
            return mask;
        });
}

// (length bits, end, m, 4 i + j) as a 96-bit key: end above m, a triangle index stays below 2^30
__device__ __forceinline__ PathKey96 record_key(const MixedRecord* x) { return PathKey96{path_key(x->length_bits, (x->end << 31) | x->m), x->kr}; }

__global__ __launch_bounds__(kBlock) void mixed_confirm_kernel(DeviceScene sc, MixedKParams mp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock]
    int* stack = &s_dyn[threadIdx.x];
    const ConfirmRow cr = confirm_row(mp.h, mp.l);
    const int lane = cr.lane, n = cr.n, row = cr.row, B = mp.h.num_bands;
    const float4 s4 = cr.s4;
    const uint32_t near = near_count(cr, mp.l);
    const uint32_t* list = mp.l.near + (size_t)cr.slot * mp.l.max_near;
    MixedRecord* conf = mp.conf + (size_t)cr.slot * mp.l.max_candidates;
    uint32_t confirmed = 0u;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {   // (wave-uniform; n > 0 only where the near list is whole)
        const int c = base + lane;
        const bool mine = c < n;
        const uint32_t code = mine ? cr.list[c] : 0u;
        const uint32_t r_code = pair_held(list, code), m_code = pair_streamed(list, code);
        const int end = (int)(pair_variant(code) & 1u);
        const int leafM = (int)(m_code >> 2);
        const Tri48 recR = sc.tris[r_code >> 2], recM = sc.tris[leafM];
        const TriEnds gr = tri_ends(recR, s4, mp.h);
        const EdgeRec er = edge_rec(gr, (int)(r_code & 3u));
        MixedCandidate f = {};
        (void)mixed_filter(mixed_edge(gr, er, r_code >> 2), mixed_face(tri_ends(recM, s4, mp.h), s4, mp.h.lis, (uint32_t)leafM), end, s4, mp.h.lis, mp.margin,
                           mp.max_detour, mp.max_length, f);
        // the first-order rule's construction at the apex: the unit normal of the edge's triangle towards Z, EZ on its side, EA beyond
        const ApexOffsets ao = apex_offsets(f.Ex, f.Ey, f.Ez, er.ox, er.oy, er.oz, er.oo, gr.nx, gr.ny, gr.nz, gr.nn, f.hZ, mp.offset);
        const float Ax = end ? s4.x : mp.h.lis[0], Ay = end ? s4.y : mp.h.lis[1], Az = end ? s4.z : mp.h.lis[2];
        const float Zx = end ? mp.h.lis[0] : s4.x, Zy = end ? mp.h.lis[1] : s4.y, Zz = end ? mp.h.lis[2] : s4.z;
        float Rx = 0.0f, Ry = 0.0f, Rz = 0.0f, d4x = 0.0f, d4y = 0.0f, d4z = 0.0f;
        bool ok = mine;
#pragma unroll 1
        for (int leg = 0; leg < 4; ++leg) {   // legs 2, 1, 3, 4 of the rule: one copy of the traversal; leg 4 starts where leg 3 ended
            if (__ballot(ok) == 0ull) break;
            const float fx = leg < 2 ? ao.upx : (leg == 2 ? ao.downx : Rx), fy = leg < 2 ? ao.upy : (leg == 2 ? ao.downy : Ry),
                        fz = leg < 2 ? ao.upz : (leg == 2 ? ao.downz : Rz);
            const float ex = (leg == 2 ? f.A1x : (leg == 3 ? Ax : Zx)) - fx, ey = (leg == 2 ? f.A1y : (leg == 3 ? Ay : Zy)) - fy,
                        ez = (leg == 2 ? f.A1z : (leg == 3 ? Az : Zz)) - fz;
            const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
            const float inv = 1.0f / len;
            const float dx = leg == 0 ? -ao.nhx : ex * inv, dy = leg == 0 ? -ao.nhy : ey * inv, dz = leg == 0 ? -ao.nhz : ez * inv;
            const float ox = leg == 3 ? fmaf(mp.offset, dx, fx) : fx, oy = leg == 3 ? fmaf(mp.offset, dy, fy) : fy, oz = leg == 3 ? fmaf(mp.offset, dz, fz) : fz;
            const float reach = leg == 0 ? 2.0f * mp.offset : (leg == 1 ? len - mp.h.pullback : (leg == 2 ? len : (len - mp.offset) - mp.h.pullback));
            const bool run = ok && !(leg == 3 && len == 0.0f);
            // legs 1, 2, 4: chain(o, d, len) with max_surfaces = 0, confirmed while reached; leg 3 ends at the first triangle that is not
            // an own actor's and asks that it be m
            AskLeaf ask{leg == 2 ? leafM : -1};
            const int status = path_chain(sc, mp.h, cr.src_object, run, ox, oy, oz, dx, dy, dz, reach, stack, ask);
            ok = run && (leg == 2 ? ask.hit : status == kChainReached);
            if (leg == 2) { Rx = ask.Px; Ry = ask.Py; Rz = ask.Pz; }
            if (leg == 3) { d4x = dx; d4y = dy; d4z = dz; }
        }
        const unsigned long long votes = __ballot(ok);
        if (ok) {
            MixedRecord* o = conf + confirmed + compact_slot(votes, lane);
            const float il = 1.0f / f.lL;
            o->length_bits = __float_as_uint(f.length);
            o->end = (uint32_t)end;
            o->m = __float_as_uint(recM.c.z);
            o->kr = __float_as_uint(recR.c.z) * 4u + (r_code & 3u);
            o->apex[0] = f.Ex; o->apex[1] = f.Ey; o->apex[2] = f.Ez;
            o->point[0] = Rx; o->point[1] = Ry; o->point[2] = Rz;
            o->direction[0] = end ? f.vx * il : -d4x; o->direction[1] = end ? f.vy * il : -d4y; o->direction[2] = end ? f.vz * il : -d4z;
            o->detour = f.length - row_distance(s4, mp.h.lis);
            o->bend_detour = f.bend;
            o->cos_bend = ((f.ux * f.vx + f.uy * f.vy) + f.uz * f.vz) / (f.lS * f.lL);
            o->material[0] = __float_as_uint(recM.c.y); o->material[1] = __float_as_uint(recR.c.y);
            o->kept = 0u;
        }
        confirmed += (uint32_t)__popcll(votes);
    }
    __syncthreads();   // the list is in memory for every lane of the wave that wrote it
    const float mm = mp.merge * mp.merge;
    const uint32_t found = mark_kept(conf, confirmed, lane, [](const MixedRecord* x) { return record_key(x); },
                                     [&](const MixedRecord& me, const MixedRecord* x) {
        const float qx = me.apex[0] - x->apex[0], qy = me.apex[1] - x->apex[1], qz = me.apex[2] - x->apex[2];
        return me.end == x->end && me.m == x->m && ((qx * qx + qy * qy) + qz * qz) < mm;
    });
    __syncthreads();
    if (!cr.row_ok) return;
    const uint32_t returned = min(found, (uint32_t)mp.max_paths);
    fs_mixed_path* out = mp.paths + (size_t)row * mp.max_paths;
#pragma unroll 1
    for (uint32_t base = 0u; base < confirmed; base += 64u) {   // the rank among the kept
        const uint32_t e = base + (uint32_t)lane;
        if (e >= confirmed) continue;
        const MixedRecord me = conf[e];
        if (me.kept == 0u) continue;
        const uint32_t rank = rank_among(confirmed, record_key(&me), [&](uint32_t j) {
            const MixedRecord* x = conf + j;
            return x->kept != 0u ? record_key(x) : PathKey96{kNoPathKey, ~0u};
        });
        if (rank >= (uint32_t)mp.max_paths) continue;
        fs_mixed_path* o = out + rank;
        const float length = __uint_as_float(me.length_bits);
        o->length = length;
        o->delay = path_delay(mp.h, length);
        o->detour = me.detour;
        o->bend_detour = me.bend_detour;
        o->cos_bend = me.cos_bend;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o->apex[k] = me.apex[k]; o->point[k] = me.point[k]; o->direction[k] = me.direction[k]; }
        o->end = me.end;
        o->triangle[0] = me.m; o->triangle[1] = me.kr >> 2;
        o->edge = me.kr & 3u;
        o->material[0] = me.material[0]; o->material[1] = me.material[1];
        const float* gm = specular_gain(sc, me.material[0], B);
#pragma unroll
        for (int b = 0; b < FS_MAX_BANDS; ++b)
            o->gain[b] = b < B ? (gm != nullptr ? gm[b] : 1.0f) * (1.0f / sqrtf(3.0f + mp.k[b] * me.bend_detour)) : 0.0f;
    }
    zero_tail(out, lane, returned, mp.max_paths);
    if (lane == 0) {
        fs_mixed_row* r = mp.rows + row;
        r->near = near;
        r->candidates = cr.cands;
        r->confirmed = confirmed;
        r->found = found;
        r->returned = returned;
        r->flags = pair_row_flags(cr, mp.l, near, FS_MIXED_NEAR_OVERFLOW, FS_MIXED_OVERFLOW);
    }
}

}  // namespace

void launch_mixed_paths(const DeviceScene& sc, const MixedKParams& mp, hipStream_t s) {
    launch_near_pair_confirm(mixed_near_kernel, mixed_pair_kernel, mixed_confirm_kernel, sc, mp, 4, mp.l.max_near, 0, s);   // a triangle: three edge records and a face
}

}  // namespace fs
