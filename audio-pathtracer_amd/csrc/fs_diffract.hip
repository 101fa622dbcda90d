// fs_diffract.hip — fs_update_diffraction_paths: the first-order edge diffraction of every source of a tick.  The definitions
// (filter, the three legs, the merge, the row) are those of include/frequensee.h, operation by operation; this file is their mapping
// onto the device, in two kernels — the construction of fs_reflect.hip with another filter and three legs instead of two.
//   diffract_scan_kernel: one thread per triangle record, loaded once; the call's source rows are staged in LDS (a broadcast), the
// listener is a kernel argument.  The three edges are filtered in registers for each row (what they share — normal, plane distances —
// is computed once); a survivor takes a place in the row's candidate list by atomicAdd on the row's counter and stores leaf position
// * 4 + edge.  The counter keeps counting past the cap: `candidates` is exact, an overflowed row is recognised in any order.
//   diffract_confirm_kernel: one wave per source row, kBlock / 64 rows per workgroup; the lanes stride over the row's candidates
// (at most FS_MAX_DIFFRACTION_CANDIDATES / 64 = 32 rounds).  A lane recomputes its candidate's values with the filter's own code —
// the same bits — and runs the legs, the short one first, as wave-convergent loops round the lane-private trav_run<false>; a lane
// whose candidate has already failed idles along with an empty cursor, a round in which no lane is left skips the remaining legs.
// Nothing is kept per candidate: a confirmed one takes the next place of the row's list in the call's device staging (ballot and
// prefix count, no atomics), written and read by the row's own wave only.  The merge and the ranks are counted over that list — a
// handful of entries — in two passes: dropped or not, then the rank among the kept.  Plain vector stores, no sort network.
//   Dynamic LDS of the confirm kernel: the stack rows [stack_rows][kBlock], nothing else.
#include "fs_dev_trav.hpp"
#include "fs_launch.hpp"

namespace fs {
namespace {

constexpr uint32_t kDiffNoObject = FS_NO_OBJECT;

// what step 1 hands on to the legs and the row
struct DiffCandidate {
    float E0x, E0y, E0z;   // the apex
    float ux, uy, uz, lS;  // u = S - E0
    float vx, vy, vz, lL;  // v = E0 - L
    float length, detour;
    float ox, oy, oz, oo;  // o = cross(w, n)
    float nx, ny, nz, nn, hS;
};

// Step 1 of the rule for one (triangle record, edge, source row)
__device__ __forceinline__ bool diffract_filter(const float4 a, const float4 b, const float4 c, int edge, float Sx, float Sy, float Sz, uint32_t so,
                                                const float (&L)[3], uint32_t lo, float m, float max_detour, DiffCandidate& f) {
    const float v0x = a.x, v0y = a.y, v0z = a.z;
    const float e1x = a.w, e1y = b.x, e1z = b.y;
    const float e2x = b.z, e2y = b.w, e2z = c.x;
    const uint32_t object = __float_as_uint(c.w);
    const bool own = object != kDiffNoObject && (object == so || object == lo);
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float nn = (nx * nx + ny * ny) + nz * nz;
    const float tx = L[0] - v0x, ty = L[1] - v0y, tz = L[2] - v0z;
    const float hL = (tx * nx + ty * ny) + tz * nz;
    const float sx = Sx - v0x, sy = Sy - v0y, sz = Sz - v0z;
    const float hS = (sx * nx + sy * ny) + sz * nz;
    const bool opposite = (hS > 0.0f && hL < 0.0f) || (hS < 0.0f && hL > 0.0f);
    const float ax = edge == 0 ? v0x : (edge == 1 ? v0x + e1x : v0x + e2x);
    const float ay = edge == 0 ? v0y : (edge == 1 ? v0y + e1y : v0y + e2y);
    const float az = edge == 0 ? v0z : (edge == 1 ? v0z + e1z : v0z + e2z);
    const float wx = edge == 0 ? e1x : (edge == 1 ? e2x - e1x : -e2x);
    const float wy = edge == 0 ? e1y : (edge == 1 ? e2y - e1y : -e2y);
    const float wz = edge == 0 ? e1z : (edge == 1 ? e2z - e1z : -e2z);
    const float ww = (wx * wx + wy * wy) + wz * wz;
    const float ox = wy * nz - wz * ny, oy = wz * nx - wx * nz, oz = wx * ny - wy * nx;
    const float oo = (ox * ox + oy * oy) + oz * oz;
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
    const float gx = Sx - L[0], gy = Sy - L[1], gz = Sz - L[2];
    const float distance = sqrtf((gx * gx + gy * gy) + gz * gz);
    const float detour = length - distance;
    const float s = hS / (hS - hL);
    const float Xx = fmaf(s, L[0] - Sx, Sx), Xy = fmaf(s, L[1] - Sy, Sy), Xz = fmaf(s, L[2] - Sz, Sz);
    const float qx = Xx - E0x, qy = Xy - E0y, qz = Xz - E0z;
    const float shadow = (qx * ox + qy * oy) + qz * oz;
    f.E0x = E0x; f.E0y = E0y; f.E0z = E0z;
    f.ux = ux; f.uy = uy; f.uz = uz; f.lS = lS;
    f.vx = vx; f.vy = vy; f.vz = vz; f.lL = lL;
    f.length = length; f.detour = detour;
    f.ox = ox; f.oy = oy; f.oz = oz; f.oo = oo;
    f.nx = nx; f.ny = ny; f.nz = nz; f.nn = nn; f.hS = hS;
    return !own && nn != 0.0f && opposite && ww != 0.0f && oo != 0.0f && sum != 0.0f && t >= -m && t <= 1.0f + m && lS != 0.0f && lL != 0.0f &&
           detour <= max_detour && shadow <= 0.0f;
}

__global__ __launch_bounds__(kBlock) void diffract_scan_kernel(DeviceScene sc, DiffractKParams dp) {
    __shared__ float4 s_src[FS_MAX_DIFFRACTION_BATCH];
    for (int r = (int)threadIdx.x; r < dp.count; r += kBlock) s_src[r] = dp.src[r];
    __syncthreads();
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= sc.num_tris) return;
    const Tri48 rec = sc.tris[i];
#pragma unroll 1
    for (int r = 0; r < dp.count; ++r) {
        const float4 s4 = s_src[r];
#pragma unroll
        for (int edge = 0; edge < 3; ++edge) {
            DiffCandidate f;
            if (diffract_filter(rec.a, rec.b, rec.c, edge, s4.x, s4.y, s4.z, __float_as_uint(s4.w), dp.lis, dp.lis_object, dp.margin, dp.max_detour, f)) {
                const uint32_t k = atomicAdd(&dp.counters[r], 1u);
                if (k < (uint32_t)dp.max_candidates) dp.cand[(size_t)r * dp.max_candidates + k] = (uint32_t)i * 4u + (uint32_t)edge;
            }
        }
    }
}

// One leg for every lane of the wave at once: chain(o, d, len) of "direct paths" with max_surfaces = 0; `active` = this lane has a
// leg to run.  true = reached with crossed == 0: nothing but triangles of the own actors within len (passed with adv = t + step,
// chain's rule 6).  (!(rem > 0) ends a leg as reached before its query: a query with such a tmax has no hit.)
__device__ __forceinline__ bool diffract_leg(const DeviceScene& sc, const DiffractKParams& dp, uint32_t src_object, bool active,
                                             float ox, float oy, float oz, float dx, float dy, float dz, float len, int* stack) {
    bool reached = false, live = active;
    float rem = len;
#pragma unroll 1
    for (int q = 0; q < FS_DIRECT_MAX_QUERIES; ++q) {
        if (live && !(rem > 0.0f)) { reached = true; live = false; }
        if (__ballot(live) == 0ull) break;
        const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
        Trav tv;
        trav_init(tv, rem, live && sc.num_nodes > 0);
        trav_deep_reset(sc, stack);
        trav_run<false>(sc, r, tv, stack);
        if (!live) continue;
        if (tv.leaf_index < 0) { reached = true; live = false; continue; }
        const uint32_t object = __float_as_uint(sc.tris[tv.leaf_index].c.w);
        const bool own = object != kDiffNoObject && (object == src_object || object == dp.lis_object);
        if (!own) { live = false; continue; }
        const float adv = tv.t + dp.step;
        ox = fmaf(adv, dx, ox); oy = fmaf(adv, dy, oy); oz = fmaf(adv, dz, oz);
        rem = rem - adv;
        if (q + 1 == FS_DIRECT_MAX_QUERIES) live = false;   // out of queries: blocked
    }
    return reached;
}

__global__ __launch_bounds__(kBlock) void diffract_confirm_kernel(DeviceScene sc, DiffractKParams dp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock]
    int* stack = &s_dyn[threadIdx.x];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int maxc = dp.max_candidates, B = dp.num_bands;
    const int row = (int)(blockIdx.x * (kBlock / 64)) + wave;
    const bool row_ok = row < dp.count;
    const float4 s4 = dp.src[row_ok ? row : 0];
    const uint32_t src_object = __float_as_uint(s4.w);
    const uint32_t cands = row_ok ? dp.counters[row] : 0u;
    const bool overflow = cands > (uint32_t)maxc;
    const int n = overflow ? 0 : (int)cands;
    const uint32_t* list = dp.cand + (size_t)(row_ok ? row : 0) * maxc;
    DiffractRecord* conf = dp.conf + (size_t)(row_ok ? row : 0) * maxc;
    uint32_t confirmed = 0u;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {   // (wave-uniform)
        const int c = base + lane;
        const bool mine = c < n;
        const uint32_t code = mine ? list[c] : 0u;
        const Tri48 rec = sc.tris[code >> 2];
        DiffCandidate f;
        (void)diffract_filter(rec.a, rec.b, rec.c, (int)(code & 3u), s4.x, s4.y, s4.z, src_object, dp.lis, dp.lis_object, dp.margin, dp.max_detour, f);
        const float io = 1.0f / sqrtf(f.oo);
        const float in = 1.0f / sqrtf(f.nn);
        const float sg = f.hS > 0.0f ? in : -in;
        const float nhx = f.nx * sg, nhy = f.ny * sg, nhz = f.nz * sg;
        const float Eox = fmaf(dp.offset, f.ox * io, f.E0x), Eoy = fmaf(dp.offset, f.oy * io, f.E0y), Eoz = fmaf(dp.offset, f.oz * io, f.E0z);
        const float ESx = fmaf(dp.offset, nhx, Eox), ESy = fmaf(dp.offset, nhy, Eoy), ESz = fmaf(dp.offset, nhz, Eoz);
        const float ELx = fmaf(-dp.offset, nhx, Eox), ELy = fmaf(-dp.offset, nhy, Eoy), ELz = fmaf(-dp.offset, nhz, Eoz);
        bool ok = mine;
#pragma unroll 1
        for (int leg = 0; leg < 3; ++leg) {   // B, A, C: one copy of the traversal; the verdicts are independent
            if (__ballot(ok) == 0ull) break;
            const float fx = leg == 0 ? ESx : (leg == 1 ? s4.x : ELx), fy = leg == 0 ? ESy : (leg == 1 ? s4.y : ELy), fz = leg == 0 ? ESz : (leg == 1 ? s4.z : ELz);
            const float ex = (leg == 1 ? ESx : dp.lis[0]) - fx, ey = (leg == 1 ? ESy : dp.lis[1]) - fy, ez = (leg == 1 ? ESz : dp.lis[2]) - fz;
            const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
            const float inv = 1.0f / len;
            const float dx = leg == 0 ? -nhx : ex * inv, dy = leg == 0 ? -nhy : ey * inv, dz = leg == 0 ? -nhz : ez * inv;
            const float reach = leg == 0 ? 2.0f * dp.offset : (leg == 1 ? len : len - dp.pullback);
            ok = diffract_leg(sc, dp, src_object, ok, fx, fy, fz, dx, dy, dz, reach, stack) && ok;
        }
        const unsigned long long votes = __ballot(ok);
        if (ok) {
            DiffractRecord* o = conf + confirmed + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
            const float il = 1.0f / f.lL;
            o->length_bits = __float_as_uint(f.length);
            o->key = __float_as_uint(rec.c.z) * 4u + (code & 3u);
            o->apex[0] = f.E0x; o->apex[1] = f.E0y; o->apex[2] = f.E0z;
            o->direction[0] = f.vx * il; o->direction[1] = f.vy * il; o->direction[2] = f.vz * il;
            o->detour = f.detour;
            o->cos_bend = ((f.ux * f.vx + f.uy * f.vy) + f.uz * f.vz) / (f.lS * f.lL);
            o->material = __float_as_uint(rec.c.y);
            o->pad = 0u;
        }
        confirmed += (uint32_t)__popcll(votes);
    }
    __syncthreads();   // the list is in memory for every lane of the wave that wrote it
    const float mm = dp.merge * dp.merge;
    uint32_t found = 0u;
#pragma unroll 1
    for (uint32_t base = 0u; base < confirmed; base += 64u) {   // dropped or kept
        const uint32_t e = base + (uint32_t)lane;
        bool kept = e < confirmed;
        if (kept) {
            const DiffractRecord me = conf[e];
            const unsigned long long key = ((unsigned long long)me.length_bits << 32) | me.key;
            for (uint32_t j = 0u; j < confirmed; ++j) {
                const DiffractRecord* x = conf + j;
                const float qx = me.apex[0] - x->apex[0], qy = me.apex[1] - x->apex[1], qz = me.apex[2] - x->apex[2];
                const float qq = (qx * qx + qy * qy) + qz * qz;
                if ((((unsigned long long)x->length_bits << 32) | x->key) < key && qq < mm) kept = false;
            }
            conf[e].pad = kept ? 1u : 0u;
        }
        found += (uint32_t)__popcll(__ballot(kept));
    }
    __syncthreads();
    if (!row_ok) return;
    const uint32_t returned = min(found, (uint32_t)dp.max_paths);
    fs_diffraction_path* out = dp.paths + (size_t)row * dp.max_paths;
#pragma unroll 1
    for (uint32_t base = 0u; base < confirmed; base += 64u) {   // the rank among the kept
        const uint32_t e = base + (uint32_t)lane;
        if (e >= confirmed) continue;
        const DiffractRecord me = conf[e];
        if (me.pad == 0u) continue;
        const unsigned long long key = ((unsigned long long)me.length_bits << 32) | me.key;
        uint32_t rank = 0u;
        for (uint32_t j = 0u; j < confirmed; ++j) {
            const DiffractRecord* x = conf + j;
            rank += (x->pad != 0u && (((unsigned long long)x->length_bits << 32) | x->key) < key) ? 1u : 0u;
        }
        if (rank >= (uint32_t)dp.max_paths) continue;
        fs_diffraction_path* o = out + rank;
        const float length = __uint_as_float(me.length_bits);
        o->length = length;
        o->delay = (length / dp.dist_divisor) / dp.sound_speed;
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
    if ((uint32_t)lane >= returned && lane < dp.max_paths) {   // the entries beyond `returned`: zero bytes
        uint32_t* z = reinterpret_cast<uint32_t*>(out + lane);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(fs_diffraction_path) / sizeof(uint32_t)); ++k) z[k] = 0u;
    }
    if (lane == 0) {
        fs_diffraction_row* r = dp.rows + row;
        r->candidates = cands;
        r->confirmed = confirmed;
        r->found = found;
        r->returned = returned;
        r->flags = overflow ? FS_DIFFRACTION_OVERFLOW : 0u;
    }
}

}  // namespace

void launch_diffraction_paths(const DeviceScene& sc_in, const DiffractKParams& dp, hipStream_t s) {
    if (dp.count <= 0) return;
    const uint32_t blocks = (uint32_t)((dp.count + kBlock / 64 - 1) / (kBlock / 64));
    DeviceScene sc = sc_in;
    if (!attach_deep(sc, blocks)) return;
    if (sc.num_tris > 0)
        hipLaunchKernelGGL(diffract_scan_kernel, dim3((uint32_t)((sc.num_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, sc, dp);
    const size_t lds = stack_bytes(sc);
    allow_lds(diffract_confirm_kernel, lds);
    hipLaunchKernelGGL(diffract_confirm_kernel, dim3(blocks), dim3(kBlock), lds, s, sc, dp);
}

}  // namespace fs
