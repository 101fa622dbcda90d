// fs_reflect.hip — fs_update_reflection_paths: the first-order specular reflections of every source of a tick.  The definitions
// (filter, leg 1, leg 2, the row) are those of include/frequensee.h, operation by operation; this file is their mapping onto the
// device, in two kernels.
//   reflect_scan_kernel: one thread per triangle record, loaded once; the call's source rows are staged in LDS (every lane reads
// the same row: a broadcast), the listener is a kernel argument.  The filter runs in registers for each row; a survivor — rare —
// takes a place in the row's candidate list by atomicAdd on the row's counter.  An index past the cap is dropped while the counter
// still counts, so `candidates` is exact and an overflowed row is recognised whatever order the triangles arrived in.
//   reflect_confirm_kernel: one wave per source row, kBlock / 64 rows per workgroup as in direct_paths_kernel; the lanes stride over
// the row's candidates (at most FS_MAX_REFLECTION_CANDIDATES / 64 rounds).  A lane recomputes its candidate's D with the filter's
// own code, then runs leg 1 and leg 2 as loops of dependent closest-hit queries in which the whole wave meets at every query: the
// lane-private traversal (trav_run<false>, the one trace_rays_kernel runs and tests/test_gpu_parity.py holds to the oracle's scan
// bit for bit) is a wave-uniform loop, a lane without work idles along with an empty cursor.  The results wait in LDS by candidate
// slot; a confirmed one finds its rank by counting the smaller (length bits, input index) keys of its row, and ranks below
// max_paths store their path.  No sort network, no atomics.
//   Dynamic LDS of the confirm kernel: the stack rows [stack_rows][kBlock] | per wave kReflFields rows of max_candidates words.
#include "fs_dev_trav.hpp"
#include "fs_launch.hpp"

namespace fs {
namespace {

constexpr uint32_t kReflNoObject = FS_NO_OBJECT;
constexpr int kReflFields = 9;   // length bits | input index | material | P | d
constexpr int kLegFree = 0, kLegTarget = 1, kLegBlocked = 2;

// Step 1 of the rule for one (triangle record, source row); D is what the legs start from.
__device__ __forceinline__ bool reflect_filter(const float4 a, const float4 b, const float4 c, float Sx, float Sy, float Sz, uint32_t so,
                                               const float (&L)[3], uint32_t lo, float m, float& Dx, float& Dy, float& Dz) {
    const float v0x = a.x, v0y = a.y, v0z = a.z;
    const float e1x = a.w, e1y = b.x, e1z = b.y;
    const float e2x = b.z, e2y = b.w, e2z = c.x;
    const uint32_t object = __float_as_uint(c.w);
    const bool own = object != kReflNoObject && (object == so || object == lo);
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float nn = (nx * nx + ny * ny) + nz * nz;
    const float tx = L[0] - v0x, ty = L[1] - v0y, tz = L[2] - v0z;
    const float hL = (tx * nx + ty * ny) + tz * nz;
    const float sx = Sx - v0x, sy = Sy - v0y, sz = Sz - v0z;
    const float hS = (sx * nx + sy * ny) + sz * nz;
    const bool side = (hS > 0.0f && hL > 0.0f) || (hS < 0.0f && hL < 0.0f);
    const float k = (2.0f * hS) / nn;
    const float Mx = Sx - k * nx, My = Sy - k * ny, Mz = Sz - k * nz;   // S'
    Dx = Mx - L[0]; Dy = My - L[1]; Dz = Mz - L[2];
    const float px = Dy * e2z - Dz * e2y, py = Dz * e2x - Dx * e2z, pz = Dx * e2y - Dy * e2x;
    const float det = (e1x * px + e1y * py) + e1z * pz;
    const float inv = 1.0f / det;
    const float u = ((tx * px + ty * py) + tz * pz) * inv;
    const float qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
    const float v = ((Dx * qx + Dy * qy) + Dz * qz) * inv;
    const float s = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
    return !own && nn != 0.0f && side && det != 0.0f && u >= -m && v >= -m && (u + v) <= 1.0f + m && s > 0.0f && s < 1.0f;
}

__global__ __launch_bounds__(kBlock) void reflect_scan_kernel(DeviceScene sc, ReflectKParams rp) {
    __shared__ float4 s_src[FS_MAX_REFLECTION_BATCH];
    for (int r = (int)threadIdx.x; r < rp.count; r += kBlock) s_src[r] = rp.src[r];
    __syncthreads();
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= sc.num_tris) return;
    const Tri48 rec = sc.tris[i];
#pragma unroll 1
    for (int r = 0; r < rp.count; ++r) {
        const float4 s4 = s_src[r];
        float Dx, Dy, Dz;
        if (reflect_filter(rec.a, rec.b, rec.c, s4.x, s4.y, s4.z, __float_as_uint(s4.w), rp.lis, rp.lis_object, rp.margin, Dx, Dy, Dz)) {
            const uint32_t k = atomicAdd(&rp.counters[r], 1u);
            if (k < (uint32_t)rp.max_candidates) rp.cand[(size_t)r * rp.max_candidates + k] = (uint32_t)i;
        }
    }
}

// One leg for every lane of the wave at once; `active` = this lane has a leg to run.  The ray passes the triangles of the own actors
// (adv = t + step, as chain's rule 6) and ends at the first other triangle: kLegTarget if that is the record at leaf position
// `target` (t1 = the distance from the leg's start, P = the hit point), else kLegBlocked; kLegFree = nothing but own actors within
// len.  Leg 1 asks for kLegTarget; leg 2 is chain(o, d, len) with max_surfaces = 0, target = -1, and asks for kLegFree (reached with
// crossed == 0).  (!(rem > 0) ends a leg as free before its query: a query with such a tmax has no hit.)
__device__ __forceinline__ int reflect_leg(const DeviceScene& sc, const ReflectKParams& rp, uint32_t src_object, bool active, int target,
                                           float ox, float oy, float oz, float dx, float dy, float dz, float len, int* stack,
                                           float& t1, float& Px, float& Py, float& Pz) {
    int status = kLegBlocked;
    float rem = len, acc = 0.0f;
    bool live = active;
#pragma unroll 1
    for (int q = 0; q < FS_DIRECT_MAX_QUERIES; ++q) {
        if (live && !(rem > 0.0f)) { status = kLegFree; live = false; }
        if (__ballot(live) == 0ull) break;
        const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
        Trav tv;
        trav_init(tv, rem, live && sc.num_nodes > 0);
        trav_deep_reset(sc, stack);
        trav_run<false>(sc, r, tv, stack);
        if (!live) continue;
        if (tv.leaf_index < 0) { status = kLegFree; live = false; continue; }
        const uint32_t object = __float_as_uint(sc.tris[tv.leaf_index].c.w);
        const bool own = object != kReflNoObject && (object == src_object || object == rp.lis_object);
        if (!own) {
            if (tv.leaf_index == target) {
                status = kLegTarget;
                t1 = acc + tv.t;
                Px = fmaf(tv.t, dx, ox); Py = fmaf(tv.t, dy, oy); Pz = fmaf(tv.t, dz, oz);
            }
            live = false;
            continue;
        }
        const float adv = tv.t + rp.step;
        ox = fmaf(adv, dx, ox); oy = fmaf(adv, dy, oy); oz = fmaf(adv, dz, oz);
        rem = rem - adv;
        acc = acc + adv;
        if (q + 1 == FS_DIRECT_MAX_QUERIES) live = false;   // out of queries: blocked
    }
    return status;
}

__global__ __launch_bounds__(kBlock) void reflect_confirm_kernel(DeviceScene sc, ReflectKParams rp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] | per wave [kReflFields][max_candidates]
    int* stack = &s_dyn[threadIdx.x];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int maxc = rp.max_candidates, B = rp.num_bands;
    uint32_t* w = reinterpret_cast<uint32_t*>(s_dyn + (size_t)sc.stack_rows * kBlock) + (size_t)wave * kReflFields * maxc;
    const int row = (int)(blockIdx.x * (kBlock / 64)) + wave;
    const bool row_ok = row < rp.count;
    const float4 s4 = rp.src[row_ok ? row : 0];
    const uint32_t src_object = __float_as_uint(s4.w);
    const uint32_t cands = row_ok ? rp.counters[row] : 0u;
    const bool overflow = cands > (uint32_t)maxc;
    const int n = overflow ? 0 : (int)cands;
    const uint32_t* list = rp.cand + (size_t)(row_ok ? row : 0) * maxc;
    uint32_t found = 0u;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {   // (wave-uniform)
        const int c = base + lane;
        const bool mine = c < n;
        const int leaf = mine ? (int)list[c] : 0;
        const Tri48 rec = sc.tris[leaf];
        float Dx, Dy, Dz;
        (void)reflect_filter(rec.a, rec.b, rec.c, s4.x, s4.y, s4.z, src_object, rp.lis, rp.lis_object, rp.margin, Dx, Dy, Dz);
        const float len1 = sqrtf((Dx * Dx + Dy * Dy) + Dz * Dz);
        const float inv1 = 1.0f / len1;
        const float dx = Dx * inv1, dy = Dy * inv1, dz = Dz * inv1;
        float t1 = 0.0f, Px = 0.0f, Py = 0.0f, Pz = 0.0f;
        const int leg1 = reflect_leg(sc, rp, src_object, mine, leaf, rp.lis[0], rp.lis[1], rp.lis[2], dx, dy, dz, len1, stack, t1, Px, Py, Pz);
        const float ex = s4.x - Px, ey = s4.y - Py, ez = s4.z - Pz;
        const float len2 = sqrtf((ex * ex + ey * ey) + ez * ez);
        const bool second = mine && leg1 == kLegTarget && len2 != 0.0f;
        const float inv2 = 1.0f / (second ? len2 : 1.0f);
        const float d2x = ex * inv2, d2y = ey * inv2, d2z = ez * inv2;
        float t2 = 0.0f, Qx = 0.0f, Qy = 0.0f, Qz = 0.0f;
        const int leg2 = reflect_leg(sc, rp, src_object, second, -1, fmaf(rp.offset, d2x, Px), fmaf(rp.offset, d2y, Py), fmaf(rp.offset, d2z, Pz),
                                     d2x, d2y, d2z, (len2 - rp.offset) - rp.pullback, stack, t2, Qx, Qy, Qz);
        const bool ok = second && leg2 == kLegFree;
        const float length = t1 + len2;
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
    if (!row_ok) return;
    const uint32_t returned = min(found, (uint32_t)rp.max_paths);
    fs_reflection_path* out = rp.paths + (size_t)row * rp.max_paths;
#pragma unroll 1
    for (int base = 0; base < n; base += 64) {
        const int c = base + lane;
        if (c >= n || w[c] == 0xFFFFFFFFu) continue;   // (a length's bits are never all ones)
        const unsigned long long key = ((unsigned long long)w[c] << 32) | w[maxc + c];
        uint32_t rank = 0u;
        for (int j = 0; j < n; ++j) rank += ((((unsigned long long)w[j] << 32) | w[maxc + j]) < key) ? 1u : 0u;
        if (rank >= (uint32_t)rp.max_paths) continue;
        fs_reflection_path* o = out + rank;
        const float length = __uint_as_float(w[c]);
        const uint32_t mat = w[2 * maxc + c];
        o->length = length;
        o->delay = (length / rp.dist_divisor) / rp.sound_speed;
        o->point[0] = __uint_as_float(w[3 * maxc + c]); o->point[1] = __uint_as_float(w[4 * maxc + c]); o->point[2] = __uint_as_float(w[5 * maxc + c]);
        o->direction[0] = __uint_as_float(w[6 * maxc + c]); o->direction[1] = __uint_as_float(w[7 * maxc + c]); o->direction[2] = __uint_as_float(w[8 * maxc + c]);
        o->triangle = w[maxc + c];
        o->material = mat;
        // the specular gain of the lobe table; a surface without a material applies no factor (apply_segment)
        const float* g = sc.lobe_gain != nullptr && mat < (uint32_t)sc.num_materials ? sc.lobe_gain + ((size_t)mat * 3 + kLobeSpecular) * B : nullptr;
#pragma unroll
        for (int b = 0; b < FS_MAX_BANDS; ++b) o->reflectance[b] = b < B ? (g != nullptr ? g[b] : 1.0f) : 0.0f;
    }
    if ((uint32_t)lane >= returned && lane < rp.max_paths) {   // the entries beyond `returned`: zero bytes
        uint32_t* z = reinterpret_cast<uint32_t*>(out + lane);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(fs_reflection_path) / sizeof(uint32_t)); ++k) z[k] = 0u;
    }
    if (lane == 0) {
        fs_reflection_row* r = rp.rows + row;
        r->candidates = cands;
        r->found = found;
        r->returned = returned;
        r->flags = overflow ? FS_REFLECTION_OVERFLOW : 0u;
    }
}

}  // namespace

void launch_reflection_paths(const DeviceScene& sc_in, const ReflectKParams& rp, hipStream_t s) {
    if (rp.count <= 0) return;
    const uint32_t blocks = (uint32_t)((rp.count + kBlock / 64 - 1) / (kBlock / 64));
    DeviceScene sc = sc_in;
    if (!attach_deep(sc, blocks)) return;
    if (sc.num_tris > 0)
        hipLaunchKernelGGL(reflect_scan_kernel, dim3((uint32_t)((sc.num_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, sc, rp);
    const size_t lds = stack_bytes(sc) + sizeof(uint32_t) * (size_t)(kBlock / 64) * kReflFields * (size_t)rp.max_candidates;
    allow_lds(reflect_confirm_kernel, lds);
    hipLaunchKernelGGL(reflect_confirm_kernel, dim3(blocks), dim3(kBlock), lds, s, sc, rp);
}

}  // namespace fs
