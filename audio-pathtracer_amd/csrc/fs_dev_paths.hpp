// fs_dev_paths.hpp — what the six path queries (fs_direct.hip, fs_reflect.hip, fs_diffract.hip, fs_reflect2.hip, fs_diffract2.hip, fs_mixed.hip)
// share on the device: the own-actor test, chain(o, d, len) of include/frequensee.h as one wave-convergent loop, the unpacking of a
// triangle record and of its edges against a source and the listener, the scan and the pair kernels' scaffolds, the confirm kernels'
// common pieces and the launches.  Nothing here knows which query calls it: what differs between them arrives as a callable.  Every fp32 operation stands where the header's rules put it (the files are built
// with -ffp-contract=off and the tests compare bits).
#pragma once

#include "fs_dev_trav.hpp"
#include "fs_launch.hpp"

namespace fs {
namespace {

static_assert(FS_MAX_REFLECTION_BATCH == FS_MAX_DIFFRACTION_BATCH && FS_MAX_REFLECTION_BATCH == FS_MAX_REFLECTION2_BATCH &&
                  FS_MAX_REFLECTION_BATCH == FS_MAX_DIFFRACTION2_BATCH && FS_MAX_REFLECTION_BATCH == FS_MAX_MIXED_BATCH,
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
// at_hit of a leg that asks for one leaf: the chain ends at the first triangle that is not an own actor's; hit = it was `leaf`,
// t = its distance from the chain's start, P = the hit point
struct AskLeaf {
    int leaf;
    bool hit = false;
    float t = 0.0f, Px = 0.0f, Py = 0.0f, Pz = 0.0f;
    __device__ __forceinline__ bool operator()(int at, float t_hit, float acc, float ox, float oy, float oz, float dx, float dy, float dz) {
        if (at == leaf) {
            hit = true;
            t = acc + t_hit;
            Px = fmaf(t_hit, dx, ox); Py = fmaf(t_hit, dy, oy); Pz = fmaf(t_hit, dz, oz);
        }
        return false;
    }
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

// edge j of a record: start a, vector w, ww = w.w, o = cross(w, n), oo = o.o (by value, as TriEnds)
struct EdgeRec {
    float ax, ay, az, wx, wy, wz, ww;
    float ox, oy, oz, oo;
};
__device__ __forceinline__ EdgeRec edge_rec(const TriEnds g, int edge) {
    EdgeRec e;
    e.ax = edge == 0 ? g.v0x : (edge == 1 ? g.v0x + g.e1x : g.v0x + g.e2x);
    e.ay = edge == 0 ? g.v0y : (edge == 1 ? g.v0y + g.e1y : g.v0y + g.e2y);
    e.az = edge == 0 ? g.v0z : (edge == 1 ? g.v0z + g.e1z : g.v0z + g.e2z);
    e.wx = edge == 0 ? g.e1x : (edge == 1 ? g.e2x - g.e1x : -g.e2x);
    e.wy = edge == 0 ? g.e1y : (edge == 1 ? g.e2y - g.e1y : -g.e2y);
    e.wz = edge == 0 ? g.e1z : (edge == 1 ? g.e2z - g.e1z : -g.e2z);
    e.ww = (e.wx * e.wx + e.wy * e.wy) + e.wz * e.wz;
    e.ox = e.wy * g.nz - e.wz * g.ny; e.oy = e.wz * g.nx - e.wx * g.nz; e.oz = e.wx * g.ny - e.wy * g.nx;
    e.oo = (e.ox * e.ox + e.oy * e.oy) + e.oz * e.oz;
    return e;
}

// |S - L| of a row
__device__ __forceinline__ float row_distance(const float4 s4, const float (&L)[3]) {
    const float gx = s4.x - L[0], gy = s4.y - L[1], gz = s4.z - L[2];
    return sqrtf((gx * gx + gy * gy) + gz * gz);
}

// The diffraction rules' construction at an apex E on an edge (o, oo) of a triangle (n, nn): nh = the unit normal towards the side on
// which `side` (a signed plane distance) is positive, Eo = E + offset o / |o|, up = Eo + offset nh, down = Eo - offset nh.
struct ApexOffsets {
    float nhx, nhy, nhz, upx, upy, upz, downx, downy, downz;
};
__device__ __forceinline__ ApexOffsets apex_offsets(float Ex, float Ey, float Ez, float ox, float oy, float oz, float oo, float nx, float ny, float nz,
                                                    float nn, float side, float offset) {
    ApexOffsets a;
    const float io = 1.0f / sqrtf(oo), in = 1.0f / sqrtf(nn), sg = side > 0.0f ? in : -in;
    a.nhx = nx * sg; a.nhy = ny * sg; a.nhz = nz * sg;
    const float Eox = fmaf(offset, ox * io, Ex), Eoy = fmaf(offset, oy * io, Ey), Eoz = fmaf(offset, oz * io, Ez);
    a.upx = fmaf(offset, a.nhx, Eox); a.upy = fmaf(offset, a.nhy, Eoy); a.upz = fmaf(offset, a.nhz, Eoz);
    a.downx = fmaf(-offset, a.nhx, Eox); a.downy = fmaf(-offset, a.nhy, Eoy); a.downz = fmaf(-offset, a.nhz, Eoz);
    return a;
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

// ---- the pair kernels -------------------------------------------------------------------------------------------------------
// near^2 pair tests per row of a second-order query.  A thread holds one entry of the row's near list in registers (held_of(code,
// the row's source): what the test needs of it that does not depend on the other entry); the near list in the other role streams
// through LDS in tiles of kPairTile entries, each unpacked once by one thread of the tile (tile_of(code, source): four float4) and then
// read entry after entry at one address for the whole wave (an LDS broadcast).  test(held, the four float4, source) settles an
// ordered pair; a survivor takes a place in the row's candidate list by atomicAdd (the counter keeps counting past the cap) as its
// two near-list slots, 15 + 15 bits.  The row's source is read behind the early return and handed to the callables.
//   A query that pairs two kinds of record keeps both in the one near list, the kind in the code, and its test answers with a mask
// in place of a bool: bit b set = the pair is a candidate in variant b (fs_mixed.hip: the path's end), one list entry each, b in the
// two bits above the slots (pair_variant).
//   The grid is (tile of held entries, share of the LDS tiles, row): blockIdx.y strides over the LDS tiles, kPairSplit ways at most.
// With (tile, row) alone a call for one source in a 5 000-triangle room is 20 workgroups on a chip of 256 compute units; split 16
// ways it is 320.  The near count is known on the device only, so the grid is sized for the cap and a workgroup beyond the row's
// near list, or of a row whose near list overflowed, leaves at once.
constexpr int kPairTile = kBlock;   // entries per LDS tile: one per thread
constexpr int kPairSplit = 16;      // the LDS tiles of a row are shared among at most this many workgroups per tile of held entries
constexpr int kSlotBits = 15;       // a candidate = slot of the held entry << 15 | slot of the streamed one
static_assert(FS_MAX_REFLECTION2_NEAR <= 1 << kSlotBits && FS_MAX_DIFFRACTION2_NEAR <= 1 << kSlotBits && FS_MAX_MIXED_NEAR <= 1 << kSlotBits,
              "a candidate is two near-list slots of 15 bits");
// a test's verdict: emit(b << 2 kSlotBits) for the pair (bool) or for every variant b of its mask (uint32_t: two variants)
template <typename Emit>
__device__ __forceinline__ void for_each_verdict(bool passed, Emit&& emit) {
    if (passed) emit(0u);
}
template <typename Emit>
__device__ __forceinline__ void for_each_verdict(uint32_t mask, Emit&& emit) {
    if (mask & 1u) emit(0u);
    if (mask & 2u) emit(1u << (2 * kSlotBits));
}
struct PairRow {
    float4 a, b, c, d;
};
template <typename HeldOf, typename TileOf, typename Test>
__device__ __forceinline__ void pair_records(const PathKHead& h, const NearPairLists& l, HeldOf&& held_of, TileOf&& tile_of, Test&& test) {
    __shared__ float4 s_tile[4][kPairTile];
    const int row = (int)blockIdx.z;
    const uint32_t counted = l.near_counters[row];
    if (counted > (uint32_t)l.max_near || blockIdx.x * (uint32_t)kBlock >= counted) return;   // (the same for the whole workgroup)
    const int near = (int)counted;
    const uint32_t* list = l.near + (size_t)row * l.max_near;
    const float4 s4 = h.src[row];
    const int slot = (int)(blockIdx.x * kBlock + threadIdx.x);
    const bool have = slot < near;
    const auto held = held_of(list[have ? slot : 0], s4);
    const int tiles = (near + kPairTile - 1) / kPairTile;
#pragma unroll 1
    for (int t = (int)blockIdx.y; t < tiles; t += (int)gridDim.y) {
        const int first = t * kPairTile;
        __syncthreads();   // the tile before has been read
        if (first + (int)threadIdx.x < near) {
            const PairRow r = tile_of(list[first + (int)threadIdx.x], s4);
            s_tile[0][threadIdx.x] = r.a; s_tile[1][threadIdx.x] = r.b; s_tile[2][threadIdx.x] = r.c; s_tile[3][threadIdx.x] = r.d;
        }
        __syncthreads();
        const int n = min(kPairTile, near - first);
        if (!have) continue;
#pragma unroll 1
        for (int j = 0; j < n; ++j) {   // (j is the same in every lane: each read below is one address per wave)
            const PairRow r = {s_tile[0][j], s_tile[1][j], s_tile[2][j], s_tile[3][j]};
            if (first + j != slot)
                for_each_verdict(test(held, r, s4), [&](uint32_t variant) {
                    const uint32_t k = atomicAdd(&l.counters[row], 1u);
                    if (k < (uint32_t)l.max_candidates)
                        l.cand[(size_t)row * l.max_candidates + k] = variant | ((uint32_t)slot << kSlotBits) | (uint32_t)(first + j);
                });
        }
    }
}
// the two near-list entries of a candidate, and its variant
__device__ __forceinline__ uint32_t pair_held(const uint32_t* list, uint32_t code) { return list[(code >> kSlotBits) & ((1u << kSlotBits) - 1u)]; }
__device__ __forceinline__ uint32_t pair_variant(uint32_t code) { return code >> (2 * kSlotBits); }
__device__ __forceinline__ uint32_t pair_streamed(const uint32_t* list, uint32_t code) { return list[code & ((1u << kSlotBits) - 1u)]; }

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

__device__ __forceinline__ ConfirmRow confirm_row(const PathKHead& h, const NearPairLists& l) { return confirm_row(h, l.counters, l.cand, l.max_candidates); }
// a second-order row's near count and flags (near_flag and cand_flag: the query's own names for the two overflows)
__device__ __forceinline__ uint32_t near_count(const ConfirmRow& c, const NearPairLists& l) { return c.row_ok ? l.near_counters[c.row] : 0u; }
__device__ __forceinline__ uint32_t pair_row_flags(const ConfirmRow& c, const NearPairLists& l, uint32_t near, uint32_t near_flag, uint32_t cand_flag) {
    return near > (uint32_t)l.max_near ? near_flag : (c.overflow ? cand_flag : 0u);
}

// the place of a confirmed lane among its round's confirmed ones: the votes of the lanes below it
__device__ __forceinline__ uint32_t compact_slot(unsigned long long votes, int lane) { return (uint32_t)__popcll(votes & ((1ull << lane) - 1ull)); }

// the specular gains of a material in the lobe table; null = a surface without a material, which applies no factor (apply_segment)
__device__ __forceinline__ const float* specular_gain(const DeviceScene& sc, uint32_t material, int B) {
    return sc.lobe_gain != nullptr && material < (uint32_t)sc.num_materials ? sc.lobe_gain + ((size_t)material * 3 + kLobeSpecular) * B : nullptr;
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

// The merge of a row's `confirmed` records, by the row's own wave: an entry is dropped when an entry of a smaller key lies close to it.
// Sets every entry's `kept` word and returns how many were kept.
template <typename Record, typename KeyOf, typename Close>
__device__ __forceinline__ uint32_t mark_kept(Record* conf, uint32_t confirmed, int lane, KeyOf&& key_of, Close&& close) {
    uint32_t found = 0u;
#pragma unroll 1
    for (uint32_t base = 0u; base < confirmed; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        bool kept = e < confirmed;
        if (kept) {
            const Record me = conf[e];
            const auto key = key_of(&me);
            for (uint32_t j = 0u; j < confirmed; ++j) {
                const Record* x = conf + j;
                if (key_of(x) < key && close(me, x)) kept = false;
            }
            conf[e].kept = kept ? 1u : 0u;
        }
        found += (uint32_t)__popcll(__ballot(kept));
    }
    return found;
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

// The scan over the triangle records, then — a second-order query (pair != nullptr) — the pair tests over the rows' near lists, of
// which a triangle record can contribute near_per_tri entries, then the confirmation of the rows with confirm_lds bytes of LDS
// behind the stack rows.
template <typename P>
inline void launch_near_pair_confirm(void (*scan)(DeviceScene, P), void (*pair)(DeviceScene, P), void (*confirm)(DeviceScene, P), const DeviceScene& sc_in,
                                     const P& p, long long near_per_tri, int max_near, size_t confirm_lds, hipStream_t s) {
    if (p.h.count <= 0) return;
    const uint32_t blocks = row_blocks(p.h.count);
    DeviceScene sc = sc_in;
    if (!attach_deep(sc, blocks)) return;
    if (sc.num_tris > 0) {
        hipLaunchKernelGGL(scan, dim3((uint32_t)((sc.num_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, sc, p);
        if (pair != nullptr) {
            const uint32_t tiles = (uint32_t)((std::min(near_per_tri * (long long)sc.num_tris, (long long)max_near) + kBlock - 1) / kBlock);
            hipLaunchKernelGGL(pair, dim3(tiles, std::min(tiles, (uint32_t)kPairSplit), (uint32_t)p.h.count), dim3(kBlock), 0, s, sc, p);
        }
    }
    const size_t lds = stack_bytes(sc) + confirm_lds;
    allow_lds(confirm, lds);
    hipLaunchKernelGGL(confirm, dim3(blocks), dim3(kBlock), lds, s, sc, p);
}
template <typename P>
inline void launch_scan_confirm(void (*scan)(DeviceScene, P), void (*confirm)(DeviceScene, P), const DeviceScene& sc, const P& p, size_t confirm_lds,
                                hipStream_t s) {
    launch_near_pair_confirm<P>(scan, nullptr, confirm, sc, p, 0, 0, confirm_lds, s);
}

}  // namespace
}  // namespace fs
