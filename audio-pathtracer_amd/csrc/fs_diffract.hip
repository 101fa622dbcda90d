// fs_diffract.hip — fs_update_diffraction_paths: the first-order edge diffraction of every source of a tick.  The definitions
// (filter, the three legs, the merge, the row) are those of include/frequensee.h, operation by operation; this file is their mapping
// onto the device, in two kernels on the scaffolds of fs_dev_paths.hpp.
//   diffract_scan_kernel: the scan scaffold (scan_records) with this file's filter.  The three edges of a record are filtered in
// registers for each row (what they share — normal, plane distances — is unpacked once); a survivor's code is leaf position * 4 + edge.
//   diffract_confirm_kernel: one wave per source row, kBlock / 64 rows per workgroup; the lanes stride over the row's candidates
// (at most FS_MAX_DIFFRACTION_CANDIDATES / 64 = 32 rounds).  A lane recomputes its candidate's values with the filter's own code —
// the same bits — and runs the legs, the short one first, as chains (path_chain) round one copy of the traversal; a lane
// whose candidate has already failed idles along with an empty cursor, a round in which no lane is left skips the remaining legs.
// Nothing is kept per candidate: a confirmed one takes the next place of the row's list in the call's device staging (compact_slot,
// no atomics), written and read by the row's own wave only.  The merge and the ranks are counted over that list — a handful of
// entries — in two passes: dropped or not (mark_kept), then the rank among the kept.  Plain vector stores, no sort network.
//   Dynamic LDS of the confirm kernel: the stack rows [stack_rows][kBlock], nothing else.
#include "fs_dev_paths.hpp"

namespace fs {
namespace {

// what step 1 hands on to the legs and the row
struct DiffCandidate {
    float E0x, E0y, E0z;   // the apex
    float ux, uy, uz, lS;  // u = S - E0
    float vx, vy, vz, lL;  // v = E0 - L
    float length, detour;
    float ox, oy, oz, oo;  // o = cross(w, n)
};

// the part of step 1 that the three edges of a record share beyond g: |S - L| and X, where the line S -> L meets the record's plane
struct DiffPlane {
    float distance, Xx, Xy, Xz;
};
__device__ __forceinline__ DiffPlane diffract_plane(const TriEnds g, const float4 s4, const float (&L)[3]) {
    DiffPlane p;
    p.distance = row_distance(s4, L);
    const float s = g.hS / (g.hS - g.hL);
    p.Xx = fmaf(s, L[0] - s4.x, s4.x); p.Xy = fmaf(s, L[1] - s4.y, s4.y); p.Xz = fmaf(s, L[2] - s4.z, s4.z);
    return p;
}

// Step 1 of the rule for one (triangle record, edge, source row); g and p = what the record's three edges share
__device__ __forceinline__ bool diffract_filter(const TriEnds g, const DiffPlane p, int edge, const float4 s4, const float (&L)[3], float m,
                                                float max_detour, DiffCandidate& f) {
    const float nn = g.nn, hS = g.hS, hL = g.hL;
    const float Sx = s4.x, Sy = s4.y, Sz = s4.z;
    const bool opposite = (hS > 0.0f && hL < 0.0f) || (hS < 0.0f && hL > 0.0f);
    const EdgeRec e = edge_rec(g, edge);
    const float ax = e.ax, ay = e.ay, az = e.az, wx = e.wx, wy = e.wy, wz = e.wz, ww = e.ww, ox = e.ox, oy = e.oy, oz = e.oz, oo = e.oo;
    const float rSx = Sx - ax, rSy = Sy - ay, rSz = Sz - az;
    const float rLx = L[0] - ax, rLy = L[1] - ay, rLz = L[2] - az;
    const float tS = ((rSx * wx + rSy * wy) + rSz * wz) / ww;
    const float tL = ((rLx * wx + rLy * wy) + rLz * wz) / ww;
    const float cSx = rSy * wz - rSz * wy, cSy = rSz * wx - rSx * wz, cSz = rSx * wy - rSy * wx;
    const float cLx = rLy * wz - rLz * wy, cLy = rLz * wx - rLx * wz, cLz = rLx * wy - rLy * wx;
    const float dS = sqrtf(((cSx * cSx + cSy * cSy) + cSz * cSz) / ww);
    const float dL = sqrtf(((cLx * cLx + cLy * cLy) + cLz * cLz) / ww);
    const float sum = dS + dL;
    const float t = tS + ((tL - tS) * dS) / sum;
    const float E0x = fmaf(t, wx, ax), E0y = fmaf(t, wy, ay), E0z = fmaf(t, wz, az);
    const float ux = Sx - E0x, uy = Sy - E0y, uz = Sz - E0z;
    const float vx = E0x - L[0], vy = E0y - L[1], vz = E0z - L[2];
    const float lS = sqrtf((ux * ux + uy * uy) + uz * uz);
    const float lL = sqrtf((vx * vx + vy * vy) + vz * vz);
    const float length = lS + lL;
    const float detour = length - p.distance;
    const float qx = p.Xx - E0x, qy = p.Xy - E0y, qz = p.Xz - E0z;
    const float shadow = (qx * ox + qy * oy) + qz * oz;
    f.E0x = E0x; f.E0y = E0y; f.E0z = E0z;
    f.ux = ux; f.uy = uy; f.uz = uz; f.lS = lS;
    f.vx = vx; f.vy = vy; f.vz = vz; f.lL = lL;
    f.length = length; f.detour = detour;
    f.ox = ox; f.oy = oy; f.oz = oz; f.oo = oo;
    return !g.own && nn != 0.0f && opposite && ww != 0.0f && oo != 0.0f && sum != 0.0f && t >= -m && t <= 1.0f + m && lS != 0.0f && lL != 0.0f &&
           detour <= max_detour && shadow <= 0.0f;
}

__global__ __launch_bounds__(kBlock) void diffract_scan_kernel(DeviceScene sc, DiffractKParams dp) {
    scan_records(sc, dp.h, dp.counters, dp.cand, dp.max_candidates, [&](uint32_t leaf, const TriEnds g, const float4 s4, auto&& emit) {
        const DiffPlane p = diffract_plane(g, s4, dp.h.lis);
#pragma unroll
        for (int edge = 0; edge < 3; ++edge) {
            DiffCandidate f;
            if (diffract_filter(g, p, edge, s4, dp.h.lis, dp.margin, dp.max_detour, f)) emit(leaf * 4u + (uint32_t)edge);
        }
    });
}

__global__ __launch_bounds__(kBlock) void diffract_confirm_kernel(DeviceScene sc, DiffractKParams dp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock]
    int* stack = &s_dyn[threadIdx.x];
    const ConfirmRow cr = confirm_row(dp.h, dp.counters, dp.cand, dp.max_candidates);
    const int lane = cr.lane, n = cr.n, row = cr.row, B = dp.h.num_bands;
    const float4 s4 = cr.s4;
    DiffractRecord* conf = dp.conf + (size_t)cr.slot * dp.max_candidates;
    uint32_t confirmed = 0u;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {   // (wave-uniform)
        const int c = base + lane;
        const bool mine = c < n;
        const uint32_t code = mine ? cr.list[c] : 0u;
        const Tri48 rec = sc.tris[code >> 2];
        const TriEnds g = tri_ends(rec, s4, dp.h);
        DiffCandidate f;
        (void)diffract_filter(g, diffract_plane(g, s4, dp.h.lis), (int)(code & 3u), s4, dp.h.lis, dp.margin, dp.max_detour, f);
        const ApexOffsets ao = apex_offsets(f.E0x, f.E0y, f.E0z, f.ox, f.oy, f.oz, f.oo, g.nx, g.ny, g.nz, g.nn, g.hS, dp.offset);   // towards S
        const float nhx = ao.nhx, nhy = ao.nhy, nhz = ao.nhz, ESx = ao.upx, ESy = ao.upy, ESz = ao.upz, ELx = ao.downx, ELy = ao.downy, ELz = ao.downz;
        bool ok = mine;
#pragma unroll 1
        for (int leg = 0; leg < 3; ++leg) {   // B, A, C: one copy of the traversal; the verdicts are independent
            if (__ballot(ok) == 0ull) break;
            const float fx = leg == 0 ? ESx : (leg == 1 ? s4.x : ELx), fy = leg == 0 ? ESy : (leg == 1 ? s4.y : ELy), fz = leg == 0 ? ESz : (leg == 1 ? s4.z : ELz);
            const float ex = (leg == 1 ? ESx : dp.h.lis[0]) - fx, ey = (leg == 1 ? ESy : dp.h.lis[1]) - fy, ez = (leg == 1 ? ESz : dp.h.lis[2]) - fz;
            const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
            const float inv = 1.0f / len;
            const float dx = leg == 0 ? -nhx : ex * inv, dy = leg == 0 ? -nhy : ey * inv, dz = leg == 0 ? -nhz : ez * inv;
            const float reach = leg == 0 ? 2.0f * dp.offset : (leg == 1 ? len : len - dp.h.pullback);
            // chain(o, d, len) with max_surfaces = 0: confirmed while reached (with crossed == 0)
            ok = path_chain(sc, dp.h, cr.src_object, ok, fx, fy, fz, dx, dy, dz, reach, stack, StopAtHit()) == kChainReached && ok;
        }
        const unsigned long long votes = __ballot(ok);
        if (ok) {
            DiffractRecord* o = conf + confirmed + compact_slot(votes, lane);
            const float il = 1.0f / f.lL;
            o->length_bits = __float_as_uint(f.length);
            o->key = __float_as_uint(rec.c.z) * 4u + (code & 3u);
            o->apex[0] = f.E0x; o->apex[1] = f.E0y; o->apex[2] = f.E0z;
            o->direction[0] = f.vx * il; o->direction[1] = f.vy * il; o->direction[2] = f.vz * il;
            o->detour = f.detour;
            o->cos_bend = ((f.ux * f.vx + f.uy * f.vy) + f.uz * f.vz) / (f.lS * f.lL);
            o->material = __float_as_uint(rec.c.y);
            o->kept = 0u;
        }
        confirmed += (uint32_t)__popcll(votes);
    }
    __syncthreads();   // the list is in memory for every lane of the wave that wrote it
    const float mm = dp.merge * dp.merge;
    const uint32_t found = mark_kept(conf, confirmed, lane, [](const DiffractRecord* x) { return path_key(x->length_bits, x->key); },
                                     [&](const DiffractRecord& me, const DiffractRecord* x) {
        const float qx = me.apex[0] - x->apex[0], qy = me.apex[1] - x->apex[1], qz = me.apex[2] - x->apex[2];
        return ((qx * qx + qy * qy) + qz * qz) < mm;
    });
    __syncthreads();
    if (!cr.row_ok) return;
    const uint32_t returned = min(found, (uint32_t)dp.max_paths);
    fs_diffraction_path* out = dp.paths + (size_t)row * dp.max_paths;
#pragma unroll 1
    for (uint32_t base = 0u; base < confirmed; base += 64u) {   // the rank among the kept
        const uint32_t e = base + (uint32_t)lane;
        if (e >= confirmed) continue;
        const DiffractRecord me = conf[e];
        if (me.kept == 0u) continue;
        const uint32_t rank = rank_among(confirmed, path_key(me.length_bits, me.key), [&](uint32_t j) {
            const DiffractRecord* x = conf + j;
            return x->kept != 0u ? path_key(x->length_bits, x->key) : kNoPathKey;
        });
        if (rank >= (uint32_t)dp.max_paths) continue;
        fs_diffraction_path* o = out + rank;
        const float length = __uint_as_float(me.length_bits);
        o->length = length;
        o->delay = path_delay(dp.h, length);
        o->detour = me.detour;
        o->cos_bend = me.cos_bend;
        o->apex[0] = me.apex[0]; o->apex[1] = me.apex[1]; o->apex[2] = me.apex[2];
        o->direction[0] = me.direction[0]; o->direction[1] = me.direction[1]; o->direction[2] = me.direction[2];
        o->triangle = me.key >> 2;
        o->edge = me.key & 3u;
        o->material = me.material;
#pragma unroll
        for (int b = 0; b < FS_MAX_BANDS; ++b) o->gain[b] = b < B ? 1.0f / sqrtf(3.0f + dp.k[b] * me.detour) : 0.0f;
    }
    zero_tail(out, lane, returned, dp.max_paths);
    if (lane == 0) {
        fs_diffraction_row* r = dp.rows + row;
        r->candidates = cr.cands;
        r->confirmed = confirmed;
        r->found = found;
        r->returned = returned;
        r->flags = cr.overflow ? FS_DIFFRACTION_OVERFLOW : 0u;
    }
}

}  // namespace

void launch_diffraction_paths(const DeviceScene& sc, const DiffractKParams& dp, hipStream_t s) {
    launch_scan_confirm(diffract_scan_kernel, diffract_confirm_kernel, sc, dp, 0, s);
}

}  // namespace fs
