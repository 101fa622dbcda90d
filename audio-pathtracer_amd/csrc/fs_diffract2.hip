// fs_diffract2.hip — fs_update_diffraction2_paths: the second-order edge diffraction of every source of a tick, the sound that bends
// round the two parallel rims of a thick obstacle.  The definitions (near set, pair filter, the five legs, the merge, the row) are
// those of include/frequensee.h, operation by operation; this file is their mapping onto the device, in three kernels on the
// scaffolds of fs_dev_paths.hpp.
//   diffract2_near_kernel: the scan scaffold (scan_records) with step 0 as its filter over the three edges of a record; a near edge
// record's code is leaf position * 4 + edge, the row's near list the "candidate list" of the scaffold.
//   diffract2_pair_kernel: the hot one — the pair scaffold (pair_records).  The held entry is a near edge record in the role of q (the
// source's end), with what depends on q and the row alone — tS, tL - tS, dS, their product, hS, o_q — precomputed; the streamed one a
// near edge record in the role of p (the listener's end): a, w, ww, dL, v0, hL, n, 15 words.  The parallel test (six multiplies)
// and the gap test stand before any divide or square root: they leave the pairs of parallel edges that are not one line; the apex
// ranges and the strict-side tests end the rest but for a handful.
//   diffract2_confirm_kernel: one wave per source row (confirm_row), the lanes stride over the row's candidates (at most
// FS_MAX_DIFFRACTION2_CANDIDATES / 64 = 32 rounds).  A lane recomputes its pair's values with the pair filter's own code — the same
// bits — and runs the five legs, the two short ones first, as chains (path_chain) round one copy of the traversal; a lane whose
// candidate has already failed idles along.  A confirmed one takes the next place of the row's list in the call's device staging
// (compact_slot), written and read by the row's own wave only; merge (mark_kept) and rank are counted over that list by the 96-bit
// key (length bits, p, q).  Plain vector stores, no sort network.
//   Dynamic LDS of the confirm kernel: the stack rows [stack_rows][kBlock], nothing else.
#include "fs_dev_paths.hpp"

namespace fs {
namespace {

// Step 0 of the rule for one (edge record, source row); bound = |S - L| + max_detour
__device__ __forceinline__ bool diffract2_near(const TriEnds g, const EdgeRec e, const float4 s4, const float (&L)[3], float bound) {
    const float rSx = s4.x - e.ax, rSy = s4.y - e.ay, rSz = s4.z - e.az;
    const float rLx = L[0] - e.ax, rLy = L[1] - e.ay, rLz = L[2] - e.az;
    const float la = sqrtf((rSx * rSx + rSy * rSy) + rSz * rSz);
    const float lb = sqrtf((rLx * rLx + rLy * rLy) + rLz * rLz);
    const float reach = sqrtf(e.ww);
    return !g.own && g.nn != 0.0f && e.ww != 0.0f && e.oo != 0.0f && ((la + lb) - (reach + reach)) <= bound;
}

// what the pair filter reads of q, the edge record at the source's end: nothing of it depends on p
struct PairQ {
    float ax, ay, az, wx, wy, wz, ww;
    float nx, ny, nz, v0x, v0y, v0z, hS;
    float ox, oy, oz;
    float tS, dt, dS, dtdS;   // tS, tL - tS, dS, (tL - tS) dS: S and L against q's line
    float distance;           // |S - L|: the row's, the same in every lane — it travels with q to the detour test
};
__device__ __forceinline__ PairQ pair_q(const TriEnds g, const EdgeRec e, const float4 s4, const float (&L)[3]) {
    PairQ q;
    q.ax = e.ax; q.ay = e.ay; q.az = e.az; q.wx = e.wx; q.wy = e.wy; q.wz = e.wz; q.ww = e.ww;
    q.nx = g.nx; q.ny = g.ny; q.nz = g.nz; q.v0x = g.v0x; q.v0y = g.v0y; q.v0z = g.v0z; q.hS = g.hS;
    q.ox = e.ox; q.oy = e.oy; q.oz = e.oz;
    const float rSx = s4.x - e.ax, rSy = s4.y - e.ay, rSz = s4.z - e.az;
    const float rLx = L[0] - e.ax, rLy = L[1] - e.ay, rLz = L[2] - e.az;
    q.tS = ((rSx * e.wx + rSy * e.wy) + rSz * e.wz) / e.ww;
    const float tL = ((rLx * e.wx + rLy * e.wy) + rLz * e.wz) / e.ww;
    const float cx = rSy * e.wz - rSz * e.wy, cy = rSz * e.wx - rSx * e.wz, cz = rSx * e.wy - rSy * e.wx;
    q.dS = sqrtf(((cx * cx + cy * cy) + cz * cz) / e.ww);
    q.dt = tL - q.tS;
    q.dtdS = q.dt * q.dS;
    q.distance = row_distance(s4, L);
    return q;
}

// what the pair filter reads of p, the edge record at the listener's end — 15 words (o_p is recomputed by the few pairs that get there)
struct PairP {
    float ax, ay, az, ww;
    float wx, wy, wz, dL;
    float v0x, v0y, v0z, hL;
    float nx, ny, nz;
};
__device__ __forceinline__ PairP pair_p(const TriEnds g, const EdgeRec e, const float (&L)[3]) {
    PairP p;
    p.ax = e.ax; p.ay = e.ay; p.az = e.az; p.ww = e.ww; p.wx = e.wx; p.wy = e.wy; p.wz = e.wz;
    p.v0x = g.v0x; p.v0y = g.v0y; p.v0z = g.v0z; p.hL = g.hL; p.nx = g.nx; p.ny = g.ny; p.nz = g.nz;
    const float rLx = L[0] - e.ax, rLy = L[1] - e.ay, rLz = L[2] - e.az;
    const float cx = rLy * e.wz - rLz * e.wy, cy = rLz * e.wx - rLx * e.wz, cz = rLx * e.wy - rLy * e.wx;
    p.dL = sqrtf(((cx * cx + cy * cy) + cz * cz) / e.ww);
    return p;
}

// what step 1 hands on to the legs and the row
struct Pair2 {
    float E0x, E0y, E0z, E1x, E1y, E1z;
    float ux, uy, uz, l1;   // u = S - E1
    float mx, my, mz, lm;   // m = E1 - E0
    float vx, vy, vz, l0;   // v = E0 - L
    float length, detour, g;   // g = the distance between the two edges' lines
    float opx, opy, opz;       // o_p
};

__device__ __forceinline__ bool strictly_opposite(float a, float b) { return (a > 0.0f && b < 0.0f) || (a < 0.0f && b > 0.0f); }

// Step 1 of the rule for one ordered pair (q, p) of near edge records.  The early returns change no bit: every operation is rounded
// on its own wherever it stands.
__device__ __forceinline__ bool pair2_filter(const PairQ& q, const PairP& p, const float4 s4, const float (&L)[3], float m,
                                             float min_parallel, float mm, float max_detour, Pair2& f) {
    const float c = (q.wx * p.wx + q.wy * p.wy) + q.wz * p.wz;
    if (!(c * c >= min_parallel * (q.ww * p.ww))) return false;
    const float rx = p.ax - q.ax, ry = p.ay - q.ay, rz = p.az - q.az;
    const float gx = ry * q.wz - rz * q.wy, gy = rz * q.wx - rx * q.wz, gz = rx * q.wy - ry * q.wx;
    const float gg = (gx * gx + gy * gy) + gz * gz;
    if (!(gg > mm * q.ww)) return false;
    const float g = sqrtf(gg / q.ww);
    const float dSg = q.dS + g;
    const float sum = dSg + p.dL;
    const float t1 = q.tS + q.dtdS / sum;
    if (!(sum != 0.0f && t1 >= -m && t1 <= 1.0f + m)) return false;
    const float tm = q.tS + (q.dt * dSg) / sum;
    const float E1x = fmaf(t1, q.wx, q.ax), E1y = fmaf(t1, q.wy, q.ay), E1z = fmaf(t1, q.wz, q.az);
    const float Px = fmaf(tm, q.wx, q.ax), Py = fmaf(tm, q.wy, q.ay), Pz = fmaf(tm, q.wz, q.az);
    const float bx = Px - p.ax, by = Py - p.ay, bz = Pz - p.az;
    const float t0 = ((bx * p.wx + by * p.wy) + bz * p.wz) / p.ww;
    if (!(t0 >= -m && t0 <= 1.0f + m)) return false;
    const float E0x = fmaf(t0, p.wx, p.ax), E0y = fmaf(t0, p.wy, p.ay), E0z = fmaf(t0, p.wz, p.az);
    // sides: q's triangle between S and E0, p's triangle between L and E1
    const float ax = E0x - q.v0x, ay = E0y - q.v0y, az = E0z - q.v0z;
    const float h0 = (ax * q.nx + ay * q.ny) + az * q.nz;
    if (!strictly_opposite(q.hS, h0)) return false;
    const float cx = E1x - p.v0x, cy = E1y - p.v0y, cz = E1z - p.v0z;
    const float h1 = (cx * p.nx + cy * p.ny) + cz * p.nz;
    if (!strictly_opposite(p.hL, h1)) return false;
    // shadow zones: the first-order rule's, the other apex as the far end
    const float s1 = q.hS / (q.hS - h0);
    const float X1x = fmaf(s1, E0x - s4.x, s4.x), X1y = fmaf(s1, E0y - s4.y, s4.y), X1z = fmaf(s1, E0z - s4.z, s4.z);
    const float d1x = X1x - E1x, d1y = X1y - E1y, d1z = X1z - E1z;
    if (!(((d1x * q.ox + d1y * q.oy) + d1z * q.oz) <= 0.0f)) return false;
    const float s0 = h1 / (h1 - p.hL);
    const float X0x = fmaf(s0, L[0] - E1x, E1x), X0y = fmaf(s0, L[1] - E1y, E1y), X0z = fmaf(s0, L[2] - E1z, E1z);
    const float opx = p.wy * p.nz - p.wz * p.ny, opy = p.wz * p.nx - p.wx * p.nz, opz = p.wx * p.ny - p.wy * p.nx;
    const float d0x = X0x - E0x, d0y = X0y - E0y, d0z = X0z - E0z;
    if (!(((d0x * opx + d0y * opy) + d0z * opz) <= 0.0f)) return false;
    // length
    const float ux = s4.x - E1x, uy = s4.y - E1y, uz = s4.z - E1z;
    const float mx = E1x - E0x, my = E1y - E0y, mz = E1z - E0z;
    const float vx = E0x - L[0], vy = E0y - L[1], vz = E0z - L[2];
    const float l1 = sqrtf((ux * ux + uy * uy) + uz * uz);
    const float lm = sqrtf((mx * mx + my * my) + mz * mz);
    const float l0 = sqrtf((vx * vx + vy * vy) + vz * vz);
    const float length = (l1 + lm) + l0;
    const float detour = length - q.distance;
    f.E0x = E0x; f.E0y = E0y; f.E0z = E0z; f.E1x = E1x; f.E1y = E1y; f.E1z = E1z;
    f.ux = ux; f.uy = uy; f.uz = uz; f.l1 = l1;
    f.mx = mx; f.my = my; f.mz = mz; f.lm = lm;
    f.vx = vx; f.vy = vy; f.vz = vz; f.l0 = l0;
    f.length = length; f.detour = detour; f.g = g;
    f.opx = opx; f.opy = opy; f.opz = opz;
    return l1 != 0.0f && lm != 0.0f && l0 != 0.0f && detour <= max_detour;
}

__global__ __launch_bounds__(kBlock) void diffract2_near_kernel(DeviceScene sc, Diffract2KParams dp) {
    scan_records(sc, dp.h, dp.l.near_counters, dp.l.near, dp.l.max_near, [&](uint32_t leaf, const TriEnds g, const float4 s4, auto&& emit) {
        const float bound = row_distance(s4, dp.h.lis) + dp.max_detour;
#pragma unroll
        for (int edge = 0; edge < 3; ++edge)
            if (diffract2_near(g, edge_rec(g, edge), s4, dp.h.lis, bound)) emit(leaf * 4u + (uint32_t)edge);
    });
}

__global__ __launch_bounds__(kBlock) void diffract2_pair_kernel(DeviceScene sc, Diffract2KParams dp) {
    const float mm = dp.merge * dp.merge;
    pair_records(
        dp.h, dp.l,
        [&](uint32_t code, const float4 s4) {
            const TriEnds g = tri_ends(sc.tris[code >> 2], s4, dp.h);
            return pair_q(g, edge_rec(g, (int)(code & 3u)), s4, dp.h.lis);
        },
        [&](uint32_t code, const float4 s4) {
            const TriEnds g = tri_ends(sc.tris[code >> 2], s4, dp.h);
            const PairP p = pair_p(g, edge_rec(g, (int)(code & 3u)), dp.h.lis);
            return PairRow{make_float4(p.ax, p.ay, p.az, p.ww), make_float4(p.wx, p.wy, p.wz, p.dL), make_float4(p.v0x, p.v0y, p.v0z, p.hL),
                           make_float4(p.nx, p.ny, p.nz, 0.0f)};
        },
        [&](const PairQ& q, const PairRow r, const float4 s4) {
            const PairP p = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w, r.d.x, r.d.y, r.d.z};
            Pair2 f;
            return pair2_filter(q, p, s4, dp.h.lis, dp.margin, dp.min_parallel, mm, dp.max_detour, f);
        });
}

__device__ __forceinline__ PathKey96 record_key(const Diffract2Record* x) { return PathKey96{path_key(x->length_bits, x->kp), x->kq}; }

__global__ __launch_bounds__(kBlock) void diffract2_confirm_kernel(DeviceScene sc, Diffract2KParams dp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock]
    int* stack = &s_dyn[threadIdx.x];
    const ConfirmRow cr = confirm_row(dp.h, dp.l);
    const int lane = cr.lane, n = cr.n, row = cr.row, B = dp.h.num_bands;
    const float4 s4 = cr.s4;
    const uint32_t near = near_count(cr, dp.l);
    const uint32_t* list = dp.l.near + (size_t)cr.slot * dp.l.max_near;
    Diffract2Record* conf = dp.conf + (size_t)cr.slot * dp.l.max_candidates;
    const float mm = dp.merge * dp.merge;
    uint32_t confirmed = 0u;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {   // (wave-uniform; n > 0 only where the near list is whole and has two entries at least)
        const int c = base + lane;
        const bool mine = c < n;
        const uint32_t code = mine ? cr.list[c] : 0u;
        const uint32_t q_code = pair_held(list, code), p_code = pair_streamed(list, code);
        const Tri48 recQ = sc.tris[q_code >> 2], recP = sc.tris[p_code >> 2];
        const TriEnds gq = tri_ends(recQ, s4, dp.h), gp = tri_ends(recP, s4, dp.h);
        const EdgeRec eq = edge_rec(gq, (int)(q_code & 3u)), ep = edge_rec(gp, (int)(p_code & 3u));
        Pair2 f = {};
        (void)pair2_filter(pair_q(gq, eq, s4, dp.h.lis), pair_p(gp, ep, dp.h.lis), s4, dp.h.lis, dp.margin, dp.min_parallel, mm,
                           dp.max_detour, f);
        // the first-order rule's construction at each edge: the unit normal of q towards S, of p towards L
        const ApexOffsets aq = apex_offsets(f.E1x, f.E1y, f.E1z, eq.ox, eq.oy, eq.oz, eq.oo, gq.nx, gq.ny, gq.nz, gq.nn, gq.hS, dp.offset);
        const ApexOffsets ap = apex_offsets(f.E0x, f.E0y, f.E0z, f.opx, f.opy, f.opz, ep.oo, gp.nx, gp.ny, gp.nz, gp.nn, gp.hL, dp.offset);
        const float nqx = aq.nhx, nqy = aq.nhy, nqz = aq.nhz, ESx = aq.upx, ESy = aq.upy, ESz = aq.upz, M1x = aq.downx, M1y = aq.downy, M1z = aq.downz;
        const float npx = ap.nhx, npy = ap.nhy, npz = ap.nhz, ELx = ap.upx, ELy = ap.upy, ELz = ap.upz, M0x = ap.downx, M0y = ap.downy, M0z = ap.downz;
        bool ok = mine;
#pragma unroll 1
        for (int leg = 0; leg < 5; ++leg) {   // legs 2, 4, 3, 1, 5 of the rule: one copy of the traversal; the verdicts are independent
            if (__ballot(ok) == 0ull) break;
            const float fx = leg == 0 ? ESx : (leg == 1 ? M0x : (leg == 2 ? M1x : (leg == 3 ? s4.x : ELx)));
            const float fy = leg == 0 ? ESy : (leg == 1 ? M0y : (leg == 2 ? M1y : (leg == 3 ? s4.y : ELy)));
            const float fz = leg == 0 ? ESz : (leg == 1 ? M0z : (leg == 2 ? M1z : (leg == 3 ? s4.z : ELz)));
            const float ex = (leg == 2 ? M0x : (leg == 3 ? ESx : dp.h.lis[0])) - fx;
            const float ey = (leg == 2 ? M0y : (leg == 3 ? ESy : dp.h.lis[1])) - fy;
            const float ez = (leg == 2 ? M0z : (leg == 3 ? ESz : dp.h.lis[2])) - fz;
            const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
            const float inv = 1.0f / len;
            const float dx = leg == 0 ? -nqx : (leg == 1 ? npx : ex * inv);
            const float dy = leg == 0 ? -nqy : (leg == 1 ? npy : ey * inv);
            const float dz = leg == 0 ? -nqz : (leg == 1 ? npz : ez * inv);
            const float reach = leg < 2 ? 2.0f * dp.offset : (leg == 4 ? len - dp.h.pullback : len);
            // chain(o, d, len) with max_surfaces = 0: confirmed while reached (with crossed == 0)
            ok = path_chain(sc, dp.h, cr.src_object, ok, fx, fy, fz, dx, dy, dz, reach, stack, StopAtHit()) == kChainReached && ok;
        }
        const unsigned long long votes = __ballot(ok);
        if (ok) {
            Diffract2Record* o = conf + confirmed + compact_slot(votes, lane);
            const float il = 1.0f / f.l0;
            o->length_bits = __float_as_uint(f.length);
            o->kp = __float_as_uint(recP.c.z) * 4u + (p_code & 3u);
            o->kq = __float_as_uint(recQ.c.z) * 4u + (q_code & 3u);
            o->apex[0][0] = f.E0x; o->apex[0][1] = f.E0y; o->apex[0][2] = f.E0z;
            o->apex[1][0] = f.E1x; o->apex[1][1] = f.E1y; o->apex[1][2] = f.E1z;
            o->direction[0] = f.vx * il; o->direction[1] = f.vy * il; o->direction[2] = f.vz * il;
            o->detour = f.detour;
            o->gap = f.g;
            o->cos_bend[0] = ((f.mx * f.vx + f.my * f.vy) + f.mz * f.vz) / (f.lm * f.l0);
            o->cos_bend[1] = ((f.ux * f.mx + f.uy * f.my) + f.uz * f.mz) / (f.l1 * f.lm);
            o->material[0] = __float_as_uint(recP.c.y); o->material[1] = __float_as_uint(recQ.c.y);
            o->kept = 0u;
        }
        confirmed += (uint32_t)__popcll(votes);
    }
    __syncthreads();   // the list is in memory for every lane of the wave that wrote it
    const uint32_t found = mark_kept(conf, confirmed, lane, [](const Diffract2Record* x) { return record_key(x); },
                                     [&](const Diffract2Record& me, const Diffract2Record* x) {
        const float ax = me.apex[0][0] - x->apex[0][0], ay = me.apex[0][1] - x->apex[0][1], az = me.apex[0][2] - x->apex[0][2];
        const float bx = me.apex[1][0] - x->apex[1][0], by = me.apex[1][1] - x->apex[1][1], bz = me.apex[1][2] - x->apex[1][2];
        return ((ax * ax + ay * ay) + az * az) < mm && ((bx * bx + by * by) + bz * bz) < mm;
    });
    __syncthreads();
    if (!cr.row_ok) return;
    const uint32_t returned = min(found, (uint32_t)dp.max_paths);
    fs_diffraction2_path* out = dp.paths + (size_t)row * dp.max_paths;
#pragma unroll 1
    for (uint32_t base = 0u; base < confirmed; base += 64u) {   // the rank among the kept
        const uint32_t e = base + (uint32_t)lane;
        if (e >= confirmed) continue;
        const Diffract2Record me = conf[e];
        if (me.kept == 0u) continue;
        const uint32_t rank = rank_among(confirmed, record_key(&me), [&](uint32_t j) {
            const Diffract2Record* x = conf + j;
            return x->kept != 0u ? record_key(x) : PathKey96{kNoPathKey, ~0u};
        });
        if (rank >= (uint32_t)dp.max_paths) continue;
        fs_diffraction2_path* o = out + rank;
        const float length = __uint_as_float(me.length_bits);
        o->length = length;
        o->delay = path_delay(dp.h, length);
        o->detour = me.detour;
        o->gap = me.gap;
        o->cos_bend[0] = me.cos_bend[0]; o->cos_bend[1] = me.cos_bend[1];
#pragma unroll
        for (int k = 0; k < 3; ++k) { o->apex[0][k] = me.apex[0][k]; o->apex[1][k] = me.apex[1][k]; o->direction[k] = me.direction[k]; }
        o->triangle[0] = me.kp >> 2; o->triangle[1] = me.kq >> 2;
        o->edge[0] = me.kp & 3u; o->edge[1] = me.kq & 3u;
        o->material[0] = me.material[0]; o->material[1] = me.material[1];
#pragma unroll
        for (int b = 0; b < FS_MAX_BANDS; ++b) {
            const float r = dp.lam5[b] / me.gap;
            const float rr = r * r;
            const float c3 = (1.0f + rr) / ((1.0f / 3.0f) + rr);
            o->gain[b] = b < B ? 1.0f / sqrtf(3.0f + (dp.k[b] * c3) * me.detour) : 0.0f;
        }
    }
    zero_tail(out, lane, returned, dp.max_paths);
    if (lane == 0) {
        fs_diffraction2_row* r = dp.rows + row;
        r->near = near;
        r->candidates = cr.cands;
        r->confirmed = confirmed;
        r->found = found;
        r->returned = returned;
        r->flags = pair_row_flags(cr, dp.l, near, FS_DIFFRACTION2_NEAR_OVERFLOW, FS_DIFFRACTION2_OVERFLOW);
    }
}

}  // namespace

void launch_diffraction2_paths(const DeviceScene& sc, const Diffract2KParams& dp, hipStream_t s) {
    launch_near_pair_confirm(diffract2_near_kernel, diffract2_pair_kernel, diffract2_confirm_kernel, sc, dp, 3, dp.l.max_near, 0, s);   // a triangle: three edge records
}

}  // namespace fs
