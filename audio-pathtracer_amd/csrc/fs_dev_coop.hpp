// fs_dev_coop.hpp — the cooperative traversal (a group of lanes searches one ray breadth first) and the walk on
// cooperative waves.
#pragma once
#include "fs_dev_walk.hpp"

namespace fs {
namespace {

// ---------------------------------------------------------------------------------------------------
// Cooperative traversal (round 4): the frames a game actually issues — the reference's 1000 pairs per source, walks without
// a depth cap (ARTS.h:176, ARTS.cpp:294) — are a CHAIN of ~70 dependent closest-hit queries; their time is the latency of
// one query times the length of the longest walk, and nothing else.  On sparse waves (a wave owns 1, 2 or 4 subpaths) the
// lane-private descent with work stealing above spends ~10 us per query: every step is a 64-B node per LANE, a 4-way
// sort, three stack pushes and a round of ballots / donation boxes / mailboxes, and the parallelism only doubles per step.
// Here the G = 64 / R lanes of a group search ONE ray together, breadth first:
//   * the tree it walks is the 4-wide one folded two levels at a time into 16-WIDE nodes (fs_refit.hip: coop16_kernel) — half
//     the levels, and a query takes about as many steps as the tree has levels;
//   * the group keeps ONE stack of pending inner nodes in LDS; a step pops up to G / 16 of them, lane j takes child j & 15 of
//     node j >> 4 and fetches exactly that child's 16-byte record (CoopChild, fs_internal.hpp: the box as fp16, rounded
//     outwards, + the reference) — with ONE ds_read_b128 if the node is among the first DeviceScene.lds_nodes of the
//     array, which every workgroup stages in its LDS, else with one global_load_dwordx4 — and tests that box;
//   * the children that are hit and inner go back on the stack by a ballot + prefix count (no sort, no donation protocol);
//   * a lane whose child is a hit LEAF requests that leaf's triangles right away and tests them itself in the NEXT step,
//     in the shadow of that step's node fetch; a closer hit goes into the group's mailbox with ds_min_u64 on the
//     (t bits << 32 | triangle id) key — the (t, id) order of the closest-hit rule — and the mailbox's t is the bound every
//     lane prunes with from the next step on.
// Without pruning order this visits more boxes than the sorted descent, with lanes that would idle anyway; a step is one
// record fetch + ~50 instructions, and a query takes about as many steps as the tree has levels.  The closest hit
// is the minimum of the key over ALL triangles the ray hits within tmax (boxes only prune, and these are supersets of the
// quantised ones), so the result is the one of trav_shared and of the oracle's brute-force scan, bit for bit, whatever
// the visiting order.
// The stack cannot overflow: a step pops k nodes and pushes at most 16 k; k is the full G / 16 only while that leaves room
// for the tree's worst-case one-node-at-a-time descent (DeviceScene.stack_need) on top, else the group descends one
// node per step (LIFO: from a stack of n entries such a descent never holds more than n + stack_need).
// LDS of a workgroup: [lds_nodes][16] CoopChild | per wave: kCoopCap pending-node words (divided among the R groups), R rays
// of 8 words, R mailboxes (u64 key, leaf).
// ---------------------------------------------------------------------------------------------------
constexpr int kCoopCap = 1024;
constexpr int kCoopMaxGroups = 4;
constexpr int kCoopRayWords = 12;    // origin, direction, reciprocals, tmax, ignored actor, -
constexpr int kCoopBoxWords = 8;     // mailbox: key (u64), hit leaf, - | unit normal of the hit triangle, its material
constexpr int kCoopRngWords = 64 * 4 + kCoopMaxGroups * 4;   // the walk's Philox words of the next bounces, one uint4 per lane | (pair, side, seed, first bounce) per group
constexpr int kCoopWaveWords = kCoopCap + kCoopMaxGroups * kCoopRayWords + kCoopMaxGroups * kCoopBoxWords + kCoopRngWords;
constexpr size_t kCoopWaveBytes = sizeof(int) * (size_t)kCoopWaveWords;
// the first words of the workgroup's dynamic LDS: the resident records.  Every thread of the workgroup must call it.
__device__ __forceinline__ void coop_stage_nodes(const CoopView& cv, int* s_dyn) {
    const uint4* src = reinterpret_cast<const uint4*>(cv.rec);
    uint4* dst = reinterpret_cast<uint4*>(s_dyn);
    for (int i = threadIdx.x; i < (cv.lds_nodes << cv.wshift); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}
// this wave's words behind the staged records
__device__ __forceinline__ int* coop_wave_words(const CoopView& cv, int* s_dyn) {
    return s_dyn + (((size_t)cv.lds_nodes << cv.wshift) * 4) + (size_t)(threadIdx.x >> 6) * kCoopWaveWords;
}

// LDS words other lanes of the wave write: typed address-space-3 accesses (ds_read / ds_write; a `volatile` generic pointer
// makes the compiler emit flat loads with system scope and a full s_waitcnt vmcnt(0) behind each — which also waits for
// every triangle record in flight), relaxed wave-scope atomics so that nothing is cached in a register across a step.
typedef __attribute__((address_space(3))) int LdsInt;
typedef __attribute__((address_space(3))) unsigned long long LdsU64;
__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load((const LdsInt*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void lds_st(int* p, int v) { __hip_atomic_store((LdsInt*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ unsigned long long lds_ld64(const unsigned long long* p) { return __hip_atomic_load((const LdsU64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void lds_st64(unsigned long long* p, unsigned long long v) { __hip_atomic_store((LdsU64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void lds_min64(unsigned long long* p, unsigned long long v) { (void)__hip_atomic_fetch_min((LdsU64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// one triangle (leaf-order index `leaf`) against the group's ray; a closer hit updates the lane's own best
// best_surf: the unit normal and the material of the lane's best triangle — computed from the record in hand with the
// builders' own operation sequence (fs_bvh.cpp / fs_build.hip / update_tris_kernel: the stored normal is exactly this), so
// that the walker needs neither the normal array nor the record again
template <bool IGN>
__device__ __forceinline__ bool coop_tri(const float4 a, const float4 b, const float4 c, const Ray& r, const float bound, const uint32_t ign,
                                         const int leaf, unsigned long long& best_key, int& best_leaf, float4& best_surf) {
    float t = 0.0f;
    bool hit = tri_hit(a, b, c, r, bound, t);
    if (IGN) hit = hit & (__float_as_uint(c.w) != ign);
    const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | __float_as_uint(c.z);
    const bool better = hit & (key < best_key);
    best_key = better ? key : best_key;
    best_leaf = better ? leaf : best_leaf;
    if (better) {
        const float e1x = a.w, e1y = b.x, e1z = b.y, e2x = b.z, e2y = b.w, e2z = c.x;
        const float nx = fmaf(e1y, e2z, -(e1z * e2y));
        const float ny = fmaf(e1z, e2x, -(e1x * e2z));
        const float nz = fmaf(e1x, e2y, -(e1y * e2x));
        const float l2 = nx * nx + ny * ny + nz * nz;
        const float inv = 1.0f / sqrtf(l2);
        best_surf = make_float4(nx * inv, ny * inv, nz * inv, c.y);
    }
    return better;
}

// The records are requested by hand, like the lane-private traversal's (trav_issue: one asm statement executed by every
// lane, the lanes that want a record selected by EXEC inside it, every destination tied in and out).  Left to the
// compiler, the loop's loads are waited for with s_waitcnt vmcnt(0) at the top of every step (its counter bookkeeping
// gives up at the loop's back edge) — i.e. the triangles requested at the end of a step land before the next step's
// node records are even requested.  By hand a step is: pop -> request the records -> s_waitcnt vmcnt(1): the triangle
// records of the previous step have landed (loads return in order and exactly the one record request is younger) -> test
// them while the records are in flight -> s_waitcnt vmcnt(0) -> boxes -> push -> request the hit leaves' triangles.
// tools/check_isa_hazards.py proves on the final ISA that nothing touches a register that is still in flight (it knows
// counted waits inside a basic block).
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4u LdsV4u;
struct CoopTris { v4f a0, b0, c0, a1, b1, c1; };
// m: the lanes that fetch from global memory (not zero).  ONE vector memory instruction, always.
__device__ __forceinline__ void coop_issue_node(const CoopView& cv, const uint32_t rec, const unsigned long long m, v4u& N) {
    const CoopChild* np = cv.rec + rec;
    unsigned long long sv;
    asm volatile("s_mov_b64 %[sv], exec\n\t"
                 "s_mov_b64 exec, %[m]\n\t"
                 "global_load_dwordx4 %[q], %[np], off\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [q] "+&v"(N), [sv] "=&s"(sv)
                 : [np] "v"(np), [m] "s"(m)
                 : "memory");
}
// m1: lanes with a hit leaf (its first triangle), m2: those whose leaf has a second one
__device__ __forceinline__ void coop_issue_tris(const DeviceScene& sc, const int first, const unsigned long long m1, const unsigned long long m2,
                                                CoopTris& X) {
    const Tri48* tp = sc.tris + (uint32_t)first;
    unsigned long long sv;
    asm volatile("s_mov_b64 %[sv], exec\n\t"
                 "s_mov_b64 exec, %[m1]\n\t"
                 "s_cbranch_execz 2f\n\t"
                 "global_load_dwordx4 %[a0], %[tp], off\n\t"
                 "global_load_dwordx4 %[b0], %[tp], off offset:16\n\t"
                 "global_load_dwordx4 %[c0], %[tp], off offset:32\n\t"
                 "s_mov_b64 exec, %[m2]\n\t"
                 "s_cbranch_execz 2f\n\t"
                 "global_load_dwordx4 %[a1], %[tp], off offset:48\n\t"
                 "global_load_dwordx4 %[b1], %[tp], off offset:64\n\t"
                 "global_load_dwordx4 %[c1], %[tp], off offset:80\n"
                 "2:\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [a0] "+&v"(X.a0), [b0] "+&v"(X.b0), [c0] "+&v"(X.c0), [a1] "+&v"(X.a1), [b1] "+&v"(X.b1), [c1] "+&v"(X.c1), [sv] "=&s"(sv)
                 : [tp] "v"(tp), [m1] "s"(m1), [m2] "s"(m2)
                 : "memory");
}
// the triangle records of the previous step have landed: exactly the one record request of coop_issue_node is younger
__device__ __forceinline__ void coop_wait_tris_behind_node(CoopTris& X) {
    asm volatile("s_waitcnt vmcnt(1)" : "+v"(X.a0), "+v"(X.b0), "+v"(X.c0), "+v"(X.a1), "+v"(X.b1), "+v"(X.c1));
}
__device__ __forceinline__ void coop_wait_all(v4u& N, CoopTris& X) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(N), "+v"(X.a0), "+v"(X.b0), "+v"(X.c0), "+v"(X.a1), "+v"(X.b1), "+v"(X.c1));
}
__device__ __forceinline__ float4 f4(const v4f v) { return make_float4(v.x, v.y, v.z, v.w); }
typedef _Float16 h2f __attribute__((ext_vector_type(2)));

// R = 1, 2 or 4 rays per wave: lane r < R owns ray r (has_ray: it has one), group r = lanes [r G, (r + 1) G) searches it.
// Every lane of the wave must call it.  Returns (owner lanes): a hit was found, T.t / T.id / T.leaf_index describe it.
// lds_nodes_base: the workgroup's staged records (coop_stage_nodes), wl: this wave's words behind them.
// surf_out (owner lanes, on a hit): the hit triangle's stored unit normal and material bits (walker_apply_hit).
template <bool IGN, bool COUNT>
__device__ __forceinline__ bool trav_coop(const DeviceScene& sc, const CoopView& cv, const int R, const bool has_ray, const Ray& own, const float tmax,
                                          const uint32_t ignore, Trav& T, const int* lds_nodes_base, int* wl, unsigned* overflow,
                                          float4* surf_out = nullptr) {
    const unsigned lane = threadIdx.x & 63u;
    const int gshift = R == 1 ? 6 : (R == 2 ? 5 : 4);
    const int G = 1 << gshift;
    const int g = (int)(lane >> gshift), j = (int)(lane & (unsigned)(G - 1));
    const int cap = kCoopCap >> (6 - gshift);
    int* stk = wl + g * cap;
    int* rayw = wl + kCoopCap;                                                                 // [group][kCoopRayWords]
    int* boxw = wl + kCoopCap + kCoopMaxGroups * kCoopRayWords;                                // [group][kCoopBoxWords]: key | leaf, - | normal, material
    unsigned long long* keyw = reinterpret_cast<unsigned long long*>(boxw);                    // (group g's key: keyw[4 g])
    T.nv = 0u; T.nt = 0u; T.sp = 0;
    T.t = tmax; T.leaf_index = -1; T.id = 0xFFFFFFFFu;
    if (sc.num_nodes <= 0) return false;                   // empty scene (wave-uniform)
#ifdef FS_WAVE_TIMELINE   // diagnostic build: T.cur = cycles before the loop, T.tri_i = in the triangle sections (wait + tests), T.tri_n = waiting for the records, T.sb = behind the loop
    const unsigned long long dbg_t0 = __builtin_amdgcn_s_memtime();
    T.cur = 0; T.tri_i = 0; T.tri_n = 0; T.sb = 0;
#endif
    if (lane < (unsigned)R) {   // the owners publish their rays, clear their mailboxes and put the root on their group's stack
        // (the ray's reciprocals travel too: the owner has them from make_ray; three v_rcp_f32 and their guards per lane and query saved)
        if (R > 1) {
            int* rw = rayw + lane * kCoopRayWords;
            lds_st(rw + 0, __float_as_int(own.ox)); lds_st(rw + 1, __float_as_int(own.oy)); lds_st(rw + 2, __float_as_int(own.oz));
            lds_st(rw + 3, __float_as_int(own.dx)); lds_st(rw + 4, __float_as_int(own.dy)); lds_st(rw + 5, __float_as_int(own.dz));
            lds_st(rw + 6, __float_as_int(own.ix)); lds_st(rw + 7, __float_as_int(own.iy)); lds_st(rw + 8, __float_as_int(own.iz));
            lds_st(rw + 9, __float_as_int(has_ray ? tmax : -1.0f));
            lds_st(rw + 10, (int)ignore);
        }
        lds_st64(keyw + 4 * lane, ((unsigned long long)__float_as_uint(tmax) << 32) | 0xFFFFFFFFull);
        lds_st(boxw + lane * kCoopBoxWords + 2, -1);
        lds_st(wl + lane * cap, 0);
    }
    __builtin_amdgcn_wave_barrier();
    const int* rw = rayw + g * kCoopRayWords;
    Ray r;
    uint32_t ign;
    int n;                                                 // pending nodes of this group (the same number in all its lanes)
    if (R == 1) {   // (wave-uniform) one ray per wave: lane 0's registers are broadcast as they are — no round trip through LDS
        auto bc = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
        r.ox = bc(own.ox); r.oy = bc(own.oy); r.oz = bc(own.oz);
        r.dx = bc(own.dx); r.dy = bc(own.dy); r.dz = bc(own.dz);
        r.ix = bc(own.ix); r.iy = bc(own.iy); r.iz = bc(own.iz);
        ign = (uint32_t)__builtin_amdgcn_readfirstlane((int)ignore);
        n = __builtin_amdgcn_readfirstlane((has_ray && tmax > 0.0f) ? 1 : 0);
    } else {
        r.ox = __int_as_float(lds_ld(rw + 0)); r.oy = __int_as_float(lds_ld(rw + 1)); r.oz = __int_as_float(lds_ld(rw + 2));
        r.dx = __int_as_float(lds_ld(rw + 3)); r.dy = __int_as_float(lds_ld(rw + 4)); r.dz = __int_as_float(lds_ld(rw + 5));
        r.ix = __int_as_float(lds_ld(rw + 6)); r.iy = __int_as_float(lds_ld(rw + 7)); r.iz = __int_as_float(lds_ld(rw + 8));
        ign = (uint32_t)lds_ld(rw + 10);
        n = __int_as_float(lds_ld(rw + 9)) > 0.0f ? 1 : 0;
    }
    r.nox = -(r.ox * r.ix); r.noy = -(r.oy * r.iy); r.noz = -(r.oz * r.iz);   // as make_ray
    const unsigned long long gmask = R == 1 ? ~0ull : (((1ull << G) - 1ull) << (g * G));
    const unsigned long long below = gmask & ((1ull << lane) - 1ull);
    const int wshift = cv.wshift, per = (1 << wshift) - 1; // 16 (or 4) lanes per node: lane j takes child j & per of node j >> wshift
    const int kfull = G >> wshift;
    const int theta = cap - (cv.stack_need + 8);           // the stack may grow to here by wide steps
    const int wide_to = theta - per * kfull;               // with n <= wide_to a full step cannot pass theta
    const int* bound_w = boxw + g * kCoopBoxWords + 1;      // high word of the mailbox key = closest t so far
    const bool negx = r.ix < 0.0f, negy = r.iy < 0.0f, negz = r.iz < 0.0f;
    unsigned long long best_key = ~0ull;                   // this lane's own closest hit
    int best_leaf = -1;
    float4 best_surf = make_float4(0.f, 0.f, 0.f, 0.f);
    int pfirst = 0, pcnt = 0;                              // the leaf whose triangles this lane requested in the previous step
    v4u N = {0u, 0u, 0u, 0u};
    CoopTris X;
    X.a0 = v4f{0.f, 0.f, 0.f, 0.f}; X.b0 = X.a0; X.c0 = X.a0; X.a1 = X.a0; X.b1 = X.a0; X.c1 = X.a0;
    const int q = j >> wshift, c = j & per;
    const int resident = cv.lds_nodes;
#if defined(FS_WAVE_TIMELINE) && !defined(FS_WAVE_TIMELINE_FINE)
    T.cur = (int)(__builtin_amdgcn_s_memtime() - dbg_t0);
#endif
    while (true) {
#ifdef FS_WAVE_TIMELINE
        ++T.sp;                                            // diagnostic build: steps of this query (T.sp is not used here otherwise)
#endif
#ifdef FS_WAVE_TIMELINE_FINE
        const unsigned long long fine_top = __builtin_amdgcn_s_memtime();
#endif
        const float bound = __int_as_float(lds_ld(bound_w));
        // ---- pop: up to G / 4 nodes, fewer when the stack is close to the room the worst-case descent needs
        int kw = kfull;
        if (n > wide_to) { const int room = theta - n; kw = room >= per ? room / per : 1; }
        const int k = n < kw ? n : kw;
        const bool act = q < k;
        const int ref = act ? lds_ld(stk + (n - 1 - q)) : 0;
#ifdef FS_WAVE_TIMELINE_FINE   // (finer split of a step: T.cur = pop until the stack entry is here, T.sb = boxes + pushes + leaf requests)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const unsigned long long fine_t0 = __builtin_amdgcn_s_memtime();
        T.cur += (int)(fine_t0 - fine_top);
#endif
        const uint32_t rec = ((uint32_t)ref << wshift) + (uint32_t)c;
        const bool in_lds = ref < resident;
        // (exactly one request in every step, whatever the lanes need — the counted wait below relies on it: when every
        // record is resident, or only triangles are left, lane 0 fetches record 0 once more)
        const unsigned long long m_glob = __ballot(act && !in_lds);
        coop_issue_node(cv, rec, m_glob != 0ull ? m_glob : 1ull, N);
        v4u L = {0u, 0u, 0u, 0u};
        if (act && in_lds) {
            L = *reinterpret_cast<const LdsV4u*>((const LdsInt*)lds_nodes_base + 4u * rec);   // ds_read_b128
        }
#ifdef FS_WAVE_TIMELINE
        const unsigned long long dbg_t1 = __builtin_amdgcn_s_memtime();
#endif
        coop_wait_tris_behind_node(X);
        if (COUNT) T.nv += (act && c == 0) ? 1u : 0u;
        // ---- the triangles requested in the previous step, tested while this step's records are in flight
        auto test_pending = [&]() {
            if (pcnt > 0) {
                // (both triangles of the leaf in one straight line — two independent chains the scheduler interleaves; a leaf of one
                // triangle tests the registers' old content with a bound nothing passes)
                bool better = coop_tri<IGN>(f4(X.a0), f4(X.b0), f4(X.c0), r, bound, ign, pfirst, best_key, best_leaf, best_surf);
                better = coop_tri<IGN>(f4(X.a1), f4(X.b1), f4(X.c1), r, pcnt > 1 ? bound : -1.0f, ign, pfirst + 1, best_key, best_leaf, best_surf) | better;
                for (int i = 2; i < pcnt; ++i) {                // leaves of three and four triangles (FS_BVH_LEAF > 2 only)
                    const Tri48 x = sc.tris[pfirst + i];
                    better = coop_tri<IGN>(x.a, x.b, x.c, r, bound, ign, pfirst + i, best_key, best_leaf, best_surf) | better;
                }
                if (COUNT) T.nt += (uint32_t)pcnt;
                if (better) lds_min64(keyw + 4 * g, best_key);  // ds_min_u64: the group's closest hit so far
                pcnt = 0;
            }
        };
        test_pending();
        // ---- this lane's child box: fp16 planes, entry / exit distances as one fma per plane
#ifdef FS_WAVE_TIMELINE
        const unsigned long long dbg_t2 = __builtin_amdgcn_s_memtime();
        T.tri_i += (int)(dbg_t2 - dbg_t1);
#endif
        coop_wait_all(N, X);
#ifdef FS_WAVE_TIMELINE_FINE
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
#ifdef FS_WAVE_TIMELINE
        T.tri_n += (int)(__builtin_amdgcn_s_memtime() - dbg_t2);
#endif
#ifdef FS_WAVE_TIMELINE_FINE
        const unsigned long long fine_box = __builtin_amdgcn_s_memtime();
#endif
        const v4u rc = in_lds ? L : N;
        const uint32_t w0 = rc.x, w1 = rc.y, w2 = rc.z;   // (scalars first: __builtin_bit_cast of a vector ELEMENT reads the vector's first word for each of them)
        const h2f lxy = __builtin_bit_cast(h2f, w0), lzhx = __builtin_bit_cast(h2f, w1), hyz = __builtin_bit_cast(h2f, w2);
        const float lox = (float)lxy.x, loy = (float)lxy.y, loz = (float)lzhx.x, hix = (float)lzhx.y, hiy = (float)hyz.x, hiz = (float)hyz.y;
        const float tnx = fmaf(negx ? hix : lox, r.ix, r.nox), tfx = fmaf(negx ? lox : hix, r.ix, r.nox);
        const float tny = fmaf(negy ? hiy : loy, r.iy, r.noy), tfy = fmaf(negy ? loy : hiy, r.iy, r.noy);
        const float tnz = fmaf(negz ? hiz : loz, r.iz, r.noz), tfz = fmaf(negz ? loz : hiz, r.iz, r.noz);
        const float tn = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, 0.0f));
        const float tf = fminf(fminf(tfx, tfy), fminf(tfz, bound));
        const bool h = act & (tn <= tf);
        const int cref = (int)rc.w;
        const bool inner = h & (cref >= 0), leaf = h & (cref < 0);
        // ---- the hit inner children go back on the stack, in lane order
        const unsigned long long m_in = __ballot(inner) & gmask;
        const int pos = (n - k) + (int)__popcll(m_in & below);
        if (inner) {
            if (pos < cap) lds_st(stk + pos, cref);
            else *overflow = 1u;                            // (cannot happen while DeviceScene.stack_need is the tree's; the frame would be traced again)
        }
        n = n - k + (int)__popcll(m_in);
        n = n < cap ? n : cap;
        // ---- a hit leaf: request its triangles now, test them in the next step
        if (leaf) {
            const int code = ~cref;
            pfirst = code >> 2;
            pcnt = (code & 3) + 1;
        }
        const unsigned long long m_leaf = __ballot(leaf);
        if (m_leaf != 0ull) coop_issue_tris(sc, leaf ? pfirst : 0, m_leaf, __ballot(leaf && pcnt > 1), X);
#ifdef FS_WAVE_TIMELINE_FINE
        T.sb += (int)(__builtin_amdgcn_s_memtime() - fine_box);
#endif
        if (__ballot(n > 0) == 0ull) {
            // no group of the wave has a node left: only the triangles just requested are pending — they are tested here and now
            // instead of in another turn of the loop (an empty pop, a record request nobody needs, 64 boxes of zeros: ~ 600 cycles
            // of the ~ 9 000 of a query)
            coop_wait_all(N, X);
            test_pending();
            break;
        }
    }
    coop_wait_all(N, X);                                    // (nothing is in flight here; the compiler must know the registers are free)
#ifdef FS_WAVE_TIMELINE
    const unsigned long long dbg_t3 = __builtin_amdgcn_s_memtime();
#endif
    // ---- the mailbox holds the closest hit of the group's ray; the lane that found it says which triangle it was
    __builtin_amdgcn_wave_barrier();
    const unsigned long long fin = lds_ld64(keyw + 4 * g);
    if (R == 1) {   // (wave-uniform) one ray per wave: the finder's registers are read across, no second trip through LDS
        const unsigned long long who = __ballot(best_leaf >= 0 && best_key == fin);   // (one lane: a triangle is tested once per query)
        bool found1 = false;
        if (who != 0ull) {
            const int f = __ffsll((long long)who) - 1;
            const int leaf1 = __builtin_amdgcn_readlane(best_leaf, f);
            const float sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best_surf.x), f));
            const float sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best_surf.y), f));
            const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best_surf.z), f));
            const float sw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best_surf.w), f));
            if (lane == 0u) {
                T.t = __uint_as_float((uint32_t)(fin >> 32));
                T.id = (uint32_t)fin;
                T.leaf_index = leaf1;
                if (surf_out) *surf_out = make_float4(sx, sy, sz, sw);
                found1 = true;
            }
        }
        __builtin_amdgcn_wave_barrier();                    // (the next query's owner rewrites the mailbox)
#if defined(FS_WAVE_TIMELINE) && !defined(FS_WAVE_TIMELINE_FINE)
        T.sb = (int)(__builtin_amdgcn_s_memtime() - dbg_t3);
#endif
        return found1;
    }
    if (best_leaf >= 0 && best_key == fin) {               // (one lane: a triangle is tested once per query)
        int* bw = boxw + g * kCoopBoxWords;
        lds_st(bw + 2, best_leaf);
        lds_st(bw + 4, __float_as_int(best_surf.x)); lds_st(bw + 5, __float_as_int(best_surf.y));
        lds_st(bw + 6, __float_as_int(best_surf.z)); lds_st(bw + 7, __float_as_int(best_surf.w));
    }
    __builtin_amdgcn_wave_barrier();
    bool found = false;
    if (lane < (unsigned)R) {
        const int* bw = boxw + lane * kCoopBoxWords;
        const unsigned long long key = lds_ld64(keyw + 4 * lane);
        if ((uint32_t)key != 0xFFFFFFFFu) {
            T.t = __uint_as_float((uint32_t)(key >> 32));
            T.id = (uint32_t)key;
            T.leaf_index = lds_ld(bw + 2);
            if (surf_out) *surf_out = make_float4(__int_as_float(lds_ld(bw + 4)), __int_as_float(lds_ld(bw + 5)), __int_as_float(lds_ld(bw + 6)),
                                                  __int_as_float(lds_ld(bw + 7)));
            found = true;
        }
    }
    __builtin_amdgcn_wave_barrier();                        // (the next query's owners rewrite the rays and mailboxes)
#if defined(FS_WAVE_TIMELINE) && !defined(FS_WAVE_TIMELINE_FINE)
    T.sb = (int)(__builtin_amdgcn_s_memtime() - dbg_t3);
#endif
    return found;
}

// The walk on cooperative waves: a wave owns R = 1, 2 or 4 subpaths (its first lanes), every query is searched by the
// whole group of 64 / R lanes (trav_coop).  Same walker, records, stages and schedule as walk_sparse_body; the workgroup
// has blockDim.x / 64 waves (4 or 16: the more waves share the staged records, the more of them fit).
template <int LOBES, bool COUNT, bool EXT = false>
__device__ __forceinline__ void walk_coop_body(const uint32_t bid, const DeviceScene& sc, const CoopView& cv, const KParams& kp,
                                               const SubpathState& st, const unsigned* __restrict__ scratch,
                                               const uint32_t* __restrict__ perm, const int rays_per_wave,
                                               const WalkStage sr_in = WalkStage(), const WalkLane ln = WalkLane()) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [lds_nodes][16] records of 4 words | [waves][kCoopWaveWords]
    __shared__ unsigned s_cnt[kPlanBuckets];
    if (perm) {
        for (int i = threadIdx.x; i <= min(kp.depth, FS_MAX_DEPTH); i += blockDim.x) s_cnt[i] = scratch[1 + i];
    }
    coop_stage_nodes(cv, s_dyn);                            // (with the barrier the bucket counts need)
    const uint32_t lane = threadIdx.x & 63u;
    // (consecutive waves, consecutive slots: the eight longest walks of a frame share a CU, two to a SIMD.  Strided over the workgroups
    // instead — wave w of workgroup b = wave number w * gridDim.x + b — they have a CU each; measured: one-source tick's walk kernel
    // 243.8 -> 241.2 us, and frames of more waves than the chip holds LOSE — a workgroup then lives as long as its longest walk with seven
    // dead waves: 8-source tick 0.42 -> 0.55 ms.  Not kept)
    const uint32_t wave = bid * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t slot = wave * (uint32_t)rays_per_wave + lane;
    int* wl = coop_wave_words(cv, s_dyn);
    // the stage of this lane's walk: the launch's, or the long-walk lane's own (WalkLane; the lane's slots come first)
    WalkStage sr = sr_in;
    bool mine = true;
    if (ln.len > 0) {
        const bool in_lane = slot < lane_slots(ln, s_cnt);
        if (in_lane) { sr.begin = ln.begin; sr.end = ln.end; }
        mine = ln.mode == kLaneBoth || (ln.mode == kLaneOnly) == in_lane;
    }
    bool alive = mine && lane < (uint32_t)rays_per_wave && slot < stage_slots(sr, st, 2u * kp.num_local, s_cnt);
    Walker w;
    walker_start(w, alive ? (perm ? planned_subpath(slot, min(kp.depth, FS_MAX_DEPTH), 2u * kp.num_local, s_cnt, perm) : slot) : 0u,
                 slot, kp, st, alive && sr.begin == 0);
    if (alive && sr.begin > 0) alive = walker_resume(w, st, sr.begin);
    Ray ray = make_ray(0.f, 0.f, 0.f, 0.f, 0.f, 1.f);
    uint32_t cnt_nv = 0u, cnt_nt = 0u;
    // The Philox words of a walk's bounces depend on (seed, pair, side, bounce) alone: the 64 / R lanes of the walk's group
    // compute the words of the next 64 / R bounces at once (ten rounds of four quarter-rate multiplies each, per bounce and
    // walk otherwise: a sixth of the time between two queries), the owner picks its bounce's words out of LDS.
    const int rshift = rays_per_wave == 1 ? 6 : (rays_per_wave == 2 ? 5 : 4);
    const int RG = 1 << rshift;
    int* rngw = wl + kCoopCap + kCoopMaxGroups * (kCoopRayWords + kCoopBoxWords);   // [64] uint4 | [group] (pair, side, seed, first bounce)
    int* rngb = rngw + 64 * 4;
    int rng_k0 = -(1 << 20);                               // owner lanes: the first bounce their group's cache holds
#ifdef FS_WAVE_TIMELINE
    const unsigned long long tl_r0 = __builtin_amdgcn_s_memrealtime(), tl_c0 = __builtin_amdgcn_s_memtime();
    unsigned long long tl_trav = 0, tl_seg = 0, tl_next = 0, tl_steps = 0, tl_pro = 0, tl_tri = 0, tl_nodewait = 0, tl_epi = 0;
#endif
    while (true) {
        bool go = false;
#ifdef FS_WAVE_TIMELINE
        const unsigned long long tl_n = __builtin_amdgcn_s_memtime();
#endif
        {   // refill the Philox cache of the groups whose walk has left it (every group recomputes: the others get the words they had)
            const bool need = alive && w.k < sr.end && (w.k < rng_k0 || w.k >= rng_k0 + RG);
            if (__ballot(need) != 0ull) {
                if (lane < (uint32_t)rays_per_wave) {
                    if (need) rng_k0 = w.k;
                    int* b = rngb + lane * 4;
                    lds_st(b + 0, (int)w.pair); lds_st(b + 1, (int)w.side);
                    lds_st(b + 2, (int)(kp.item_seeds > 0 ? item_seed_lo(kp, w.li / kp.pairs_per_source) : kp.seed_lo));
                    lds_st(b + 3, rng_k0);
                }
                __builtin_amdgcn_wave_barrier();
                const int* b = rngb + (lane >> rshift) * 4;
                const uint32_t bounce = (uint32_t)(lds_ld(b + 3) + (int)(lane & (uint32_t)(RG - 1)));
                uint4 pr = philox((uint32_t)lds_ld(b + 0), (bounce << 1) | (uint32_t)lds_ld(b + 1), 0, (uint32_t)lds_ld(b + 2), kp.seed_hi);
                if (LOBES == 0 && bounce > 0u) {   // every bounce but the first leaves a surface (unless every ray so far missed: the owner
                    float lx, ly, cphi;            //   then draws its words again): the cone sample's hit-independent half, here
                    cone_local(u01(pr.y), u01(pr.z), kp.cosine, lx, ly, cphi);
                    pr.y = __float_as_uint(lx); pr.z = __float_as_uint(ly); pr.w = __float_as_uint(cphi);
                }
                lds_st(rngw + 4 * lane + 0, (int)pr.x); lds_st(rngw + 4 * lane + 1, (int)pr.y);
                lds_st(rngw + 4 * lane + 2, (int)pr.z); lds_st(rngw + 4 * lane + 3, (int)pr.w);
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (alive) {
            if (w.k >= sr.end) { walker_suspend(w, st); alive = false; }   // staged walk: the next stage goes on from here
            else {
                const int ri = 4 * (((int)lane << rshift) + (w.k - rng_k0));   // owner lane g: its group's lanes start at g * RG
                const uint4 pre = make_uint4((uint32_t)lds_ld(rngw + ri), (uint32_t)lds_ld(rngw + ri + 1), (uint32_t)lds_ld(rngw + ri + 2),
                                             (uint32_t)lds_ld(rngw + ri + 3));
                const bool cone_form = LOBES == 0 && w.k > 0;          // what the cache holds for this bounce
                go = (cone_form && !w.has_normal) ? walker_next_ray<LOBES>(w, kp, sc, st, ray)   // (all misses so far: a sphere sample from the raw words)
                                                  : walker_next_ray<LOBES>(w, kp, sc, st, ray, &pre, cone_form);
                if (!go) {
                    walker_finish<EXT>(w, st);
                    if (st.cont_b && w.k >= FS_MAX_DEPTH) st.cont_b[slot] = make_float4(0.f, 0.f, 0.f, 0.f);   // a walk of the last schedule bucket: later stages visit this slot again
                    alive = false;
                }
            }
        }
        if (__ballot(go) == 0ull) break;
        Trav T;
#ifdef FS_WAVE_TIMELINE
        const unsigned long long tl_a = __builtin_amdgcn_s_memtime();
        tl_next += tl_a - tl_n;
#endif
        float4 surf = make_float4(0.f, 0.f, 0.f, 0.f);
        trav_coop<EXT, COUNT>(sc, cv, rays_per_wave, go, ray, kp.max_trace_dist, w.ign, T, s_dyn, wl, st.overflow, &surf);
#ifdef FS_WAVE_TIMELINE
        tl_trav += __builtin_amdgcn_s_memtime() - tl_a;
        tl_steps += (unsigned long long)T.sp;
        tl_pro += (unsigned long long)T.cur; tl_tri += (unsigned long long)T.tri_i; tl_nodewait += (unsigned long long)T.tri_n; tl_epi += (unsigned long long)T.sb;
        ++tl_seg;
#endif
        if (COUNT) { cnt_nv += T.nv; cnt_nt += T.nt; }
        if (go) walker_apply_hit<EXT>(w, kp, sc, st, ray, T, &surf);
    }
    if (COUNT) add_fetch_counts(const_cast<unsigned*>(scratch), 3, cnt_nv, cnt_nt);
#ifdef FS_WAVE_TIMELINE
    if (lane == 0u && g_wave_buf) {   // [0] start, [1] end (100 MHz) | cycles: [2] in queries, [3] in all, [6] in the loop head | [4] traversal steps, [5] queries
        unsigned long long* o = g_wave_buf + 8ull * wave;
        o[0] = tl_r0; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = tl_trav;
        o[3] = __builtin_amdgcn_s_memtime() - tl_c0; o[4] = tl_steps; o[6] = tl_next;
        o[5] = tl_seg | ((unsigned long long)__builtin_amdgcn_s_getreg(((16 - 1) << 11) | (0 << 6) | 4) << 32)             // HW_REG_HW_ID bits [15:0]: wave, simd, pipe, cu, sh, se
               | ((unsigned long long)(__builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20) & 0xFu) << 48);           // HW_REG_XCC_ID
        o[7] = (tl_pro & 0xFFFFull) | ((tl_tri / 16) & 0xFFFFull) << 16 | ((tl_nodewait / 16) & 0xFFFFull) << 32 | ((tl_epi / 16) & 0xFFFFull) << 48;   // (/16, 16 bits each)
        o[7] = (tl_pro / 16 & 0xFFFFull) | (o[7] & ~0xFFFFull);
    }
#endif
}

}  // namespace
}  // namespace fs
