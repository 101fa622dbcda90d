// fs_dev_paths.hpp — what the four path queries (fs_direct.hip, fs_reflect.hip, fs_diffract.hip, fs_reflect2.hip) share on the device: the own-actor
// test, chain(o, d, len) of include/frequensee.h as one wave-convergent loop, the unpacking of a triangle record against a source
// and the listener, the scan kernels' scaffold and the confirm kernels' common pieces.  Nothing here knows which query calls it: what
// differs between them arrives as a callable.  Every fp32 operation stands where the header's rules put it (the files are built
// with -ffp-contract=off and the tests compare bits).
#pragma once

#include "fs_dev_trav.hpp"
#include "fs_launch.hpp"

namespace fs {
namespace {

static_assert(FS_MAX_REFLECTION_BATCH == FS_MAX_DIFFRACTION_BATCH && FS_MAX_REFLECTION_BATCH == FS_MAX_REFLECTION2_BATCH,
              "the scan kernels stage a call's rows in one LDS array size");
constexpr int kPathBatch = FS_MAX_REFLECTION_BATCH;
constexpr int kRowsPerBlock = kBlock / 64;   // the wave-per-row kernels: a workgroup serves kBlock / 64 rows

// a triangle of the source's or the listener's own actor: passed by every chain, never a candidate
__device__ __forceinline__ bool own_actor(uint32_t object, uint32_t so, uint32_t lo) {
    return object != FS_NO_OBJECT && (object == so || object == lo);
}

// (length / dist_divisor) / sound_speed: the delay of a row or a path
__device__ __forceinline__ float path_delay(const PathKHead& h, float length) { return (length / h.dist_divisor) / h.sound_speed; }

// ---- the chain ------------------------------------------------------------------------------------------------------
// how a lane's chain ended
constexpr int kChainIdle = 0;      // the lane had no chain to run
constexpr int kChainReached = 1;   // nothing (left) within len: !(rem > 0) before a query, or a query without a hit
constexpr int kChainStopped = 2;   // at_hit answered "stop"
constexpr int kChainSpent = 3;     // FS_DIRECT_MAX_QUERIES queries and still not at the end

// chain(o, d, len) for every lane of the wave at once; `active` = this lane has a chain to run.  A loop of dependent closest-hit
// queries in which the whole wave meets at every query: the lane-private traversal (trav_run<false>, the one trace_rays_kernel runs
// and tests/test_gpu_parity.py holds to the oracle's scan bit for bit) is a wave-uniform loop, a lane whose chain has ended or that
// never had one idles along with an empty cursor.  A triangle of the own actors is passed (adv = t + step, chain's rule 6); at any
// other one at_hit(leaf position, t, distance from the chain's start to the query's origin, the query's origin, its direction) says
// whether the chain passes through (true) or stops there (false).  (!(rem > 0) ends a chain as reached before its query: a query
// with such a tmax has no hit.)  acc is summed advance by advance — len - rem is not the same number — and costs nothing where
// at_hit ignores it.
template <typename AtHit>
__device__ __forceinline__ int path_chain(const DeviceScene& sc, const PathKHead& h, uint32_t src_object, bool active, float ox, float oy,
                                          float oz, float dx, float dy, float dz, float len, int* stack, AtHit&& at_hit) {
    int end = kChainIdle;
    float rem = len, acc = 0.0f;
    bool live = active;
#pragma unroll 1
    for (int q = 0; q < FS_DIRECT_MAX_QUERIES; ++q) {
        if (live && !(rem > 0.0f)) { end = kChainReached; live = false; }
        if (__ballot(live) == 0ull) break;
        const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
        Trav tv;
        trav_init(tv, rem, live && sc.num_nodes > 0);
        trav_deep_reset(sc, stack);
        trav_run<false>(sc, r, tv, stack);
        if (!live) continue;
        if (tv.leaf_index < 0) { end = kChainReached; live = false; continue; }
        const uint32_t object = __float_as_uint(sc.tris[tv.leaf_index].c.w);
        if (!own_actor(object, src_object, h.lis_object) && !at_hit(tv.leaf_index, tv.t, acc, ox, oy, oz, dx, dy, dz)) {
            end = kChainStopped;
            live = false;
            continue;
        }
        const float adv = tv.t + h.step;
        ox = fmaf(adv, dx, ox); oy = fmaf(adv, dy, oy); oz = fmaf(adv, dz, oz);
        rem = rem - adv;
        acc = acc + adv;
        if (q + 1 == FS_DIRECT_MAX_QUERIES) { end = kChainSpent; live = false; }
    }
    return end;
}

// at_hit of a chain with max_surfaces = 0: it ends at the first triangle that is not an own actor's
struct StopAtHit {
    __device__ __forceinline__ bool operator()(int, float, float, float, float, float, float, float, float) const { return false; }
};

// ---- a triangle record against a source and the listener ---------------------------------------------------------------
// What the reflection and the diffraction filter both start from: the record's corner and edges, its normal n = cross(e1, e2), nn = |n|^2,
// t = L - v0, the plane distances hL = t . n and hS = (S - v0) . n (unnormalised), own = a triangle of the source's or the listener's actor.
// The filters take it by value: they are inlined, and its fields are then the locals they were when each filter unpacked the record
// itself (by reference the scan loops came out a tenth longer).
struct TriEnds {
    float v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z;
    float nx, ny, nz, nn;
    float tx, ty, tz, hL, hS;
    bool own;
};
__device__ __forceinline__ TriEnds tri_ends(const Tri48& rec, const float4 s4, const PathKHead& h) {
    TriEnds g;
    g.v0x = rec.a.x; g.v0y = rec.a.y; g.v0z = rec.a.z;
    g.e1x = rec.a.w; g.e1y = rec.b.x; g.e1z = rec.b.y;
    g.e2x = rec.b.z; g.e2y = rec.b.w; g.e2z = rec.c.x;
    g.own = own_actor(__float_as_uint(rec.c.w), __float_as_uint(s4.w), h.lis_object);
    g.nx = g.e1y * g.e2z - g.e1z * g.e2y; g.ny = g.e1z * g.e2x - g.e1x * g.e2z; g.nz = g.e1x * g.e2y - g.e1y * g.e2x;
    g.nn = (g.nx * g.nx + g.ny * g.ny) + g.nz * g.nz;
    g.tx = h.lis[0] - g.v0x; g.ty = h.lis[1] - g.v0y; g.tz = h.lis[2] - g.v0z;
    g.hL = (g.tx * g.nx + g.ty * g.ny) + g.tz * g.nz;
    const float sx = s4.x - g.v0x, sy = s4.y - g.v0y, sz = s4.z - g.v0z;
    g.hS = (sx * g.nx + sy * g.ny) + sz * g.nz;
    return g;
}

// ---- the scan kernels -------------------------------------------------------------------------------------------------------
// One thread per triangle record, loaded once; the call's source rows are staged in LDS (every lane reads the same row: a
// broadcast), the listener is a kernel argument.  filter(leaf position, g, row's source, emit) runs in registers for each row and
// calls emit(code) for every survivor — rare — which takes a place in the row's candidate list by atomicAdd on the row's counter.
// An index past the cap is dropped while the counter still counts, so `candidates` is exact and an overflowed row is recognised
// whatever order the triangles arrived in.
template <typename Filter>
__device__ __forceinline__ void scan_records(const DeviceScene& sc, const PathKHead& h, uint32_t* counters, uint32_t* cand, int max_candidates,
                                             Filter&& filter) {
    __shared__ float4 s_src[kPathBatch];
    for (int r = (int)threadIdx.x; r < h.count; r += kBlock) s_src[r] = h.src[r];
    __syncthreads();
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= sc.num_tris) return;
    const Tri48 rec = sc.tris[i];
#pragma unroll 1
    for (int r = 0; r < h.count; ++r) {
        const float4 s4 = s_src[r];
        filter((uint32_t)i, tri_ends(rec, s4, h), s4, [&](uint32_t code) {
            const uint32_t k = atomicAdd(&counters[r], 1u);
            if (k < (uint32_t)max_candidates) cand[(size_t)r * max_candidates + k] = code;
        });
    }
}

// ---- the confirm kernels ----------------------------------------------------------------------------------------------------
// One wave per source row, kRowsPerBlock rows per workgroup; the lanes stride over the row's n candidates.  A wave beyond the call's
// last row runs along on row 0's source with n = 0 (slot = the row whose arrays it may index) and writes nothing.
struct ConfirmRow {
    int lane, wave, row, slot, n;
    bool row_ok, overflow;
    float4 s4;
    uint32_t src_object, cands;
    const uint32_t* list;
};
__device__ __forceinline__ ConfirmRow confirm_row(const PathKHead& h, const uint32_t* counters, const uint32_t* cand, int max_candidates) {
    ConfirmRow c;
    c.lane = (int)(threadIdx.x & 63u);
    c.wave = (int)(threadIdx.x >> 6);
    c.row = (int)(blockIdx.x * kRowsPerBlock) + c.wave;
    c.row_ok = c.row < h.count;
    c.slot = c.row_ok ? c.row : 0;
    c.s4 = h.src[c.slot];
    c.src_object = __float_as_uint(c.s4.w);
    c.cands = c.row_ok ? counters[c.row] : 0u;
    c.overflow = c.cands > (uint32_t)max_candidates;
    c.n = c.overflow ? 0 : (int)c.cands;
    c.list = cand + (size_t)c.slot * max_candidates;
    return c;
}

// the order of a row's paths: by length (its bits: lengths are positive), ties by input index (* 4 + edge)
__device__ __forceinline__ unsigned long long path_key(uint32_t length_bits, uint32_t index) { return ((unsigned long long)length_bits << 32) | index; }
constexpr unsigned long long kNoPathKey = ~0ull;   // the key of an entry that is not ranked: smaller than no path's (a length's bits are never all ones)

// the order of a path off two triangles: (length bits, a), then b — a 96-bit key
struct PathKey96 {
    unsigned long long hi;
    uint32_t lo;
};
__device__ __forceinline__ bool operator<(const PathKey96& x, const PathKey96& y) { return x.hi < y.hi || (x.hi == y.hi && x.lo < y.lo); }

// a path's rank: how many of the row's n keys are smaller.  No sort network, no atomics.
template <typename Key, typename KeyAt>
__device__ __forceinline__ uint32_t rank_among(uint32_t n, Key key, KeyAt&& key_at) {
    uint32_t rank = 0u;
    for (uint32_t j = 0u; j < n; ++j) rank += key_at(j) < key ? 1u : 0u;
    return rank;
}

// the entries beyond `returned`: zero bytes, one entry per lane
template <typename Path>
__device__ __forceinline__ void zero_tail(Path* out, int lane, uint32_t returned, int max_paths) {
    if ((uint32_t)lane >= returned && lane < max_paths) {
        uint32_t* z = reinterpret_cast<uint32_t*>(out + lane);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(Path) / sizeof(uint32_t)); ++k) z[k] = 0u;
    }
}

// ---- the launches ------------------------------------------------------------------------------------------------------------
inline uint32_t row_blocks(int count) { return (uint32_t)((count + kRowsPerBlock - 1) / kRowsPerBlock); }

// the scan over the triangle records, then the confirmation of the rows with confirm_lds bytes of LDS behind the stack rows
template <typename P>
inline void launch_scan_confirm(void (*scan)(DeviceScene, P), void (*confirm)(DeviceScene, P), const DeviceScene& sc_in, const P& p, size_t confirm_lds,
                                hipStream_t s) {
    if (p.h.count <= 0) return;
    const uint32_t blocks = row_blocks(p.h.count);
    DeviceScene sc = sc_in;
    if (!attach_deep(sc, blocks)) return;
    if (sc.num_tris > 0) hipLaunchKernelGGL(scan, dim3((uint32_t)((sc.num_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, sc, p);
    const size_t lds = stack_bytes(sc) + confirm_lds;
    allow_lds(confirm, lds);
    hipLaunchKernelGGL(confirm, dim3(blocks), dim3(kBlock), lds, s, sc, p);
}

}  // namespace
}  // namespace fs
