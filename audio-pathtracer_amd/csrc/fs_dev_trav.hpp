// fs_dev_trav.hpp — BVH traversal, one ray per lane (the resumable step, the bounded LDS stack with its deep store in
// HBM), and the wave work sharing of closest-hit and any-hit queries.
#pragma once
#include "fs_dev_common.hpp"

namespace fs {
namespace {

// ---------------------------------------------------------------------------------------------------
// BVH traversal, one ray per lane, as a resumable single loop.  Every call of trav_step a busy lane
// advances on BOTH fronts it has work on: it tests one triangle of its pending leaf AND visits its next
// inner node (4 child boxes).  A wave executes both code paths in most iterations anyway (its lanes are
// in different phases), so letting one lane use both halves the iterations a ray needs — per ray about
// max(node visits, triangle tests) instead of their sum.  The closest hit does not depend on the order
// of the tests, so results are unchanged.  A lane can be parked/resumed between any two steps.
// `stack` is this lane's column of the workgroup's LDS stack (element i at stack[i * kBlock]).
// ---------------------------------------------------------------------------------------------------

struct Trav {
    int cur;        // next node, as NodeLayout::cursor(child reference): >= 0 inner (node index / view record), < 0 leaf (decoded by
                    // NodeLayout::leaf_range alone), kDone = none
    int sp;         // stack top (entries live in [sb, sp))
    int sb;         // stack bottom: 0 unless entries were given away from the bottom (wave work sharing)
    int tri_i, tri_n;  // pending triangles [tri_i, tri_n) of the current leaf
    float t;        // closest hit so far (init: tmax)
    int leaf_index; // hit triangle: its index in the array the layout's leaf_range counts in (sc.tris as bound by the launcher), -1 = none
    uint32_t id;    // its input index (tie-break key)
    uint32_t nv, nt;   // COUNT instantiations only (fs_set_profiling level 3): node records / triangle records this lane fetched
    uint32_t ni, nl, nd;   // ... and (one lane per wave) node-request instructions, their active lanes, the distinct records among those
};

// The bound T.t is canonical (no signalling NaN) from the start: it enters here and with a taken subtree, and every
// later value is the result of a division.  The node part's min with it then needs no canonicalising v_max per visit.
__device__ __forceinline__ float canonical_bound(float t) { return __builtin_canonicalizef(t); }
__device__ __forceinline__ void trav_init(Trav& T, float tmax, bool scene_nonempty) {
    T.cur = scene_nonempty ? 0 : kDone;
    T.sp = 0; T.sb = 0; T.tri_i = 0; T.tri_n = 0;
    T.t = canonical_bound(tmax); T.leaf_index = -1; T.id = 0xFFFFFFFFu;
    T.nv = 0u; T.nt = 0u; T.ni = 0u; T.nl = 0u; T.nd = 0u;
}
__device__ __forceinline__ bool trav_busy(const Trav& T) { return T.tri_i < T.tri_n || T.cur != kDone; }
// The lanes of the wave for which `p` holds, for the masks of every step.  `p` should be ONE compare on registers: then
// the mask is the compare's own scalar result.  __ballot(int), the ballot of `a || b` and the ballot of a condition the
// compiler has traced back through branches all turn the lane mask they start from into a 0 / 1 per lane and compare
// that again (v_cndmask 0, 1 + v_cmp_ne: two vector instructions per mask).
__device__ __forceinline__ unsigned long long lane_mask(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// the number of lanes of `m` below this one (v_mbcnt: no per-lane mask of the lower lanes has to live in registers)
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// The step in pieces, ordered so that as little as possible lies between the arrival of a lane's records and the
// request for its next ones (round 3: one extra L1-hit load per step costs the walk as much as 20 more vector
// instructions — every instruction of a wave between `wait` and the next `issue` is on its serial critical path):
//   trav_wait       the records have arrived
//   trav_node_part  4 child boxes of the lane's node against the bound known so far, sort, pushes, next node
//   trav_settle     a pending leaf becomes the triangle cursor and the next node is popped right away
//   trav_issue      request the node and / or triangle record the lane needs NEXT (the triangle into the other register set)
//   trav_tri_part   test the triangle that arrived with this step — in the shadow of the fetch just issued
// The node test uses the bound from before this step's triangle test: a looser bound only admits more candidates,
// and the (t, id) key decides among them, so the closest hit is unchanged bit for bit.
// The loads are inline asm under the lanes' own exec mask, waited for once behind both groups: a lane without a
// pending triangle (or node) requests nothing, both records of a lane are in flight together.  (Round 1 let every lane
// fetch a dummy record 0 with plain loads instead, because inside `if (has_node)` / `if (has_tri)` blocks the compiler
// sinks the first arithmetic on the loaded words into the block of the loads, i.e. waits for one record before it
// requests the other: 448 lane-loads per wave iteration for 207 useful ones.)
typedef float v4f __attribute__((ext_vector_type(4)));
struct TriRegs { v4f a, b, c; };
// what the box arithmetic of a node visit needs, whichever record it came from: the origin, grid step x the ray's reciprocal
// direction per axis, the six plane words (byte c = child c's plane on the node's 8-bit grid)
struct NodeBox { float ox, oy, oz, sx, sy, sz; uint32_t lox, loy, loz, hix, hiy, hiz; };
// record index x 48 as a shift-add and a shift (left alone the compiler makes it one quarter-rate v_mul_lo_u32)
__device__ __forceinline__ uint32_t offset48(uint32_t i) {
    uint32_t o = (i << 1) + i;
    asm("" : "+v"(o));
    return o << 4;
}

// The request.  ONE asm statement, executed by every lane that reaches it, with every destination register tied in and
// out ("+v"): the lanes that want a record are selected by writing their ballot to EXEC inside the statement.  Both
// matter.  (1) The compiler does not know that the destinations are still being written until the next wait; with
// conditionally executed "=v" outputs the old and the new value meet in a phi, and register allocation is free to
// resolve that phi with copies placed right behind the request — reading registers whose data has not arrived (round 3
// lost a day's first build to exactly that; tools/check_isa_hazards.py now proves the absence of such accesses on the
// final ISA).  A tied operand chain issue -> wait -> use has no phi to resolve.  (2) Every wave executes the same
// number of vector memory instructions per step whatever its lanes need, so counted waits stay possible.
// Addresses: the record arrays' bases are wave-uniform and stay in scalar registers; a lane supplies only its 32-bit
// byte offset (the layout's node_offset, triangle index * 48) and the 16-byte quarters are the instruction's own
// offset — `global_load_dwordx4 vdst, voff, s[base:base+1] offset:n`.  No 64-bit vector arithmetic and no address pairs
// in a kernel held to 128 registers; fs_scene_commit refuses a scene whose record arrays exceed 4 GiB (DeviceScene,
// fs_internal.hpp).  (No cache-policy bits on these requests: measured, none helps — DESIGN.md section 5.)
// The statement exists once per layout, because the operand lists differ; its text — EXEC saved, set and restored, the
// three node quarters both layouts have, the triangle half — and the operands common to both are written here.
#define FS_REQUEST_ASM(MORE_NODE_LOADS)                                                                         \
    "s_mov_b64 %[sv], exec\n\t"                                                                                 \
    "s_mov_b64 exec, %[mn]\n\t"                                                                                 \
    "global_load_dwordx4 %[q0], %[no], %[nb]\n\t"                                                               \
    "global_load_dwordx4 %[q1], %[no], %[nb] offset:16\n\t"                                                     \
    "global_load_dwordx4 %[q2], %[no], %[nb] offset:32\n\t" MORE_NODE_LOADS                                     \
    "s_mov_b64 exec, %[mt]\n\t"                                                                                 \
    "s_cbranch_execz 1f\n\t" /* one wave step in four has no lane with a pending triangle */                    \
    "global_load_dwordx4 %[ta], %[to], %[tb_]\n\t"                                                              \
    "global_load_dwordx4 %[tb], %[to], %[tb_] offset:16\n\t"                                                    \
    "global_load_dwordx4 %[tc], %[to], %[tb_] offset:32\n"                                                      \
    "1:\n\t"                                                                                                    \
    "s_mov_b64 exec, %[sv]"
#define FS_REQUEST_NODE_OUT [q0] "+&v"(N.q0), [q1] "+&v"(N.q1), [q2] "+&v"(N.q2)
#define FS_REQUEST_TRI_OUT [ta] "+&v"(X.a), [tb] "+&v"(X.b), [tc] "+&v"(X.c), [sv] "=&s"(sv)
#define FS_REQUEST_IN [no] "v"(no), [to] "v"(to), [nb] "s"(sc.nodes), [tb_] "s"(sc.tris), [mn] "s"(mn), [mt] "s"(mt)
// the wait for everything requested: every register in flight is listed, tied in and out like the request's
#define FS_WAIT(...) asm volatile("s_waitcnt vmcnt(0)" : __VA_ARGS__)
#define FS_NODE3(N) "+v"(N.q0), "+v"(N.q1), "+v"(N.q2)
#define FS_TRI3(X) "+v"(X.a), "+v"(X.b), "+v"(X.c)

// ---- the two record formats a traversal can walk.  A translation unit walks ONE (NodeLayout below); everything in this
// file that differs between them is in these two structs, each to be read top to bottom on its own. ----------------------

// NodeQ4 and Tri48 (fs_internal.hpp), two arrays: a 64-byte node in four requests, child references NodeQ4::child as they are.
struct NodeLayoutQ4 {
    static constexpr bool kIsView = false;
    struct Regs { v4f q0, q1, q2, q3; };   // the node quarters in flight
    static constexpr uint32_t kMiss = 0xFFFFFFFCu;   // node test: sort key of a child the ray misses (| slot)
    static __device__ __forceinline__ int cursor(int ref) { return ref; }   // >= 0 inner index, < 0 leaf code
    static __device__ __forceinline__ void leaf_range(int cur, int& first, int& end) {   // ~cur = first * 4 + count - 1
        const int code = ~cur; first = code >> 2; end = first + (code & 3) + 1;
    }
    static_assert(sizeof(NodeQ4) == 64 && sizeof(Tri48) == 48, "the request's byte offsets");
    static __device__ __forceinline__ uint32_t node_offset(int cur) { return (uint32_t)cur << 6; }
    static __device__ __forceinline__ void request(const DeviceScene& sc, Regs& N, TriRegs& X, uint32_t no, uint32_t to,
                                                   unsigned long long mn, unsigned long long mt) {
        unsigned long long sv;
        asm volatile(FS_REQUEST_ASM("global_load_dwordx4 %[q3], %[no], %[nb] offset:48\n\t")
                     : FS_REQUEST_NODE_OUT, [q3] "+&v"(N.q3), FS_REQUEST_TRI_OUT : FS_REQUEST_IN : "memory");
    }
    static __device__ __forceinline__ void wait(Regs& N, TriRegs& X) { FS_WAIT(FS_NODE3(N), "+v"(N.q3), FS_TRI3(X)); }
    static __device__ __forceinline__ void drain(Regs& N, TriRegs& X, TriRegs& Y) { FS_WAIT(FS_NODE3(N), "+v"(N.q3), FS_TRI3(X), FS_TRI3(Y)); }
    // the record (fs_internal.hpp: NodeQ4): origin, sx | lox, loy, loz, hix | hiy, hiz, sy, sz | child[4]
    static __device__ __forceinline__ NodeBox decode(const Regs& N, const Ray& r) {
        return NodeBox{N.q0.x, N.q0.y, N.q0.z, N.q0.w * r.ix, N.q2.z * r.iy, N.q2.w * r.iz,   // grid step (a power of two) / direction
                       __float_as_uint(N.q1.x), __float_as_uint(N.q1.y), __float_as_uint(N.q1.z),
                       __float_as_uint(N.q1.w), __float_as_uint(N.q2.x), __float_as_uint(N.q2.y)};
    }
    // a hit child's key: the entry distance (>= 0, so its bits order like an integer) with the slot in the low 2 bits; a missed
    // child sorts behind every hit one (kMiss | slot)
    static __device__ __forceinline__ uint32_t hit_key(const Regs&, float tn, int c) { return (__float_as_uint(tn) & ~3u) | (uint32_t)c; }
    static __device__ __forceinline__ uint32_t miss_key(int c) { return kMiss | (uint32_t)c; }
    // sort the 4 (key, child reference) pairs, nearest first: 5-comparator network, branch-free.  (Measured in
    // round 2: choosing only the nearest child and pushing the rest in slot order — also no ordering at all for
    // visibility rays — saves a dozen instructions per visit and costs as much in extra visits: walk 0.356 ->
    // 0.361 ms, connect 0.075 -> 0.078 ms.)
    static __device__ __forceinline__ void order(const Regs& N, uint32_t (&key)[4], int& ref0, int& ref1, int& ref2, int& ref3) {
        ref0 = __float_as_int(N.q3.x); ref1 = __float_as_int(N.q3.y); ref2 = __float_as_int(N.q3.z); ref3 = __float_as_int(N.q3.w);
#define FS_CSWAP(a, b) { const bool sw_ = key[b] < key[a]; const uint32_t lo_ = min(key[a], key[b]); \
                         const uint32_t hi_ = max(key[a], key[b]); key[a] = lo_; key[b] = hi_; \
                         const int ra_ = sw_ ? ref##b : ref##a; const int rb_ = sw_ ? ref##a : ref##b; \
                         ref##a = ra_; ref##b = rb_; }
        FS_CSWAP(0, 1) FS_CSWAP(2, 3) FS_CSWAP(0, 2) FS_CSWAP(1, 3) FS_CSWAP(1, 2)
#undef FS_CSWAP
    }
    static bool bind(DeviceScene&) { return true; }   // (host) DeviceScene's arrays are this layout's
};

// The 48-byte node view (fs_internal.hpp: ViewRec and the view_* word formats): sc.nodes and sc.tris are ONE array of
// 48-byte records — a node takes three requests instead of four and its child references are  cb8 + the slot's byte,
// formed behind the sort.  On the stack, in the donation boxes and in the deep store a reference stays that opaque word;
// the cursor holds it turned (view_cursor), so that the leaf bit is the sign and every mask of the step is the one
// compare it is without the view.
struct NodeLayoutView {
    static constexpr bool kIsView = true;
    struct Regs { v4f q0, q1, q2; };   // the node quarters in flight
    static constexpr uint32_t kMiss = 0xFFFFFF00u;   // node test: a missed child's key is ~0; the low byte of a hit one is its slot byte
    static_assert(view_is_leaf(kDone) && view_count(kDone) == 1 && view_record(kDone) == 0,
                  "kDone decodes as a one-triangle leaf at record 0, which is the root: never a reference");
    static __device__ __forceinline__ int cursor(int ref) { return view_cursor((uint32_t)ref); }
    static __device__ __forceinline__ void leaf_range(int cur, int& first, int& end) { first = view_record(cur); end = first + view_count(cur); }
    static_assert(sizeof(ViewRec) == 48 && sizeof(Tri48) == 48, "the request's byte offsets: both (record x 3) << 4");
    static __device__ __forceinline__ uint32_t node_offset(int cur) { return offset48((uint32_t)cur); }
    static __device__ __forceinline__ void request(const DeviceScene& sc, Regs& N, TriRegs& X, uint32_t no, uint32_t to,
                                                   unsigned long long mn, unsigned long long mt) {
        unsigned long long sv;   // (sc.nodes == sc.tris here: both groups from the one array)
        asm volatile(FS_REQUEST_ASM("") : FS_REQUEST_NODE_OUT, FS_REQUEST_TRI_OUT : FS_REQUEST_IN : "memory");
    }
    static __device__ __forceinline__ void wait(Regs& N, TriRegs& X) { FS_WAIT(FS_NODE3(N), FS_TRI3(X)); }
    static __device__ __forceinline__ void drain(Regs& N, TriRegs& X, TriRegs& Y) { FS_WAIT(FS_NODE3(N), FS_TRI3(X), FS_TRI3(Y)); }
    // grid step K of a record: exponent byte K of E moved to the float's exponent (view_step_bits), as ONE instruction
    // (the byte select is the operand's own; written as a shift and a mask it is two per step)
    template <int K>
    static __device__ __forceinline__ float step(uint32_t E) {
        static_assert(K >= 0 && K < 3, "three steps");
        float out;
        if (K == 0) asm("v_lshlrev_b32_sdwa %0, 23, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(out) : "v"(E));
        else if (K == 1) asm("v_lshlrev_b32_sdwa %0, 23, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(out) : "v"(E));
        else asm("v_lshlrev_b32_sdwa %0, 23, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(out) : "v"(E));
        return out;
    }
    // the record (fs_internal.hpp: ViewRec): origin, lox | loy, loz, hix, hiy | hiz, G, cb8, E.  The steps come back from
    // their exponent bytes bit for bit; the box arithmetic is then the NodeQ4 path's.
    static __device__ __forceinline__ NodeBox decode(const Regs& N, const Ray& r) {
        const uint32_t E = __float_as_uint(N.q2.w);
        return NodeBox{N.q0.x, N.q0.y, N.q0.z, step<0>(E) * r.ix, step<1>(E) * r.iy, step<2>(E) * r.iz,
                       __float_as_uint(N.q0.w), __float_as_uint(N.q1.x), __float_as_uint(N.q1.y),
                       __float_as_uint(N.q1.z), __float_as_uint(N.q1.w), __float_as_uint(N.q2.x)};
    }
    // entry distance with the slot's byte of G in the low 8 bits (one v_perm_b32: bytes 3 - 1 of the distance, byte c of G):
    // the reference then comes OUT of the sort — cb8 + the sorted key's low byte — and nothing is dragged through it.
    // The order of near-equal children may differ from the NodeQ4 path's; a closest hit does not depend on the order of
    // the visits and an any-hit answer is a boolean.
    static __device__ __forceinline__ uint32_t hit_key(const Regs& N, float tn, int c) {
        return __builtin_amdgcn_perm(__float_as_uint(tn), __float_as_uint(N.q2.y), 0x07060500u + (uint32_t)c);
    }
    static __device__ __forceinline__ uint32_t miss_key(int) { return 0xFFFFFFFFu; }
    // the same 5-comparator network as NodeLayoutQ4's (why there is a sort at all: there), on the keys alone
    static __device__ __forceinline__ void order(const Regs& N, uint32_t (&key)[4], int& ref0, int& ref1, int& ref2, int& ref3) {
#define FS_KEYSWAP(a, b) { const uint32_t lo_ = min(key[a], key[b]), hi_ = max(key[a], key[b]); key[a] = lo_; key[b] = hi_; }
        FS_KEYSWAP(0, 1) FS_KEYSWAP(2, 3) FS_KEYSWAP(0, 2) FS_KEYSWAP(1, 3) FS_KEYSWAP(1, 2)
#undef FS_KEYSWAP
        const uint32_t cb8 = __float_as_uint(N.q2.z);
        ref0 = (int)view_ref(cb8, key[0] & 0xFFu); ref1 = (int)view_ref(cb8, key[1] & 0xFFu);
        ref2 = (int)view_ref(cb8, key[2] & 0xFFu); ref3 = (int)view_ref(cb8, key[3] & 0xFFu);
    }
    // (host) A unit of this layout reads ONE array: record 0 is the root, a hit's leaf_index is a record number (hit_surface
    // reads that record as the Tri48 it is, its normal from the view's parallel array).  DeviceScene keeps the pointer types
    // every other unit walks, so the array is handed over under both names; no code of this layout reads a NodeQ4 from it.
    // false: the scene has no view (too large, a step that is no power of two) and is not empty (that requests no record).
    static bool bind(DeviceScene& sc) {
        const NodeView view = sc.coop_info ? sc.coop_info->view : NodeView{};
        if (!view.rec) return sc.num_nodes <= 0;
        sc.nodes = reinterpret_cast<const NodeQ4*>(view.rec);
        sc.tris = reinterpret_cast<const Tri48*>(view.rec);
        sc.tri_nrm = view.nrm;
        return true;
    }
};
#undef FS_REQUEST_ASM
#undef FS_REQUEST_NODE_OUT
#undef FS_REQUEST_TRI_OUT
#undef FS_REQUEST_IN
#undef FS_WAIT
#undef FS_NODE3
#undef FS_TRI3

// The layout of this translation unit.  A macro and not a template parameter: a parameter would thread through some twenty
// templates (walk_shared_body, connect_body, ...) for the sake of a unit that holds both, and no product unit does.  It
// must be settled before this header is first seen: FS_TRAV_LAYOUT_CHOSEN lets a unit that tries later refuse to compile.
#define FS_TRAV_LAYOUT_CHOSEN 1
#ifdef FS_NODE_VIEW   // (fs_frame.hip: the narrow flavours of the fused frame kernel)
using NodeLayout = NodeLayoutView;
#else
using NodeLayout = NodeLayoutQ4;
#endif
using NodeRegs = NodeLayout::Regs;

// ---- bounded LDS stack with a deep store in HBM (DeviceScene.deep, fs_internal.hpp) ---------------------------
// The logical stack of a lane is  deep[0, count)  followed by  LDS rows [sb, sp).  Entries move between the two in
// chunks of kDeepChunk, oldest first out, newest first back, so pops keep their order.  All of it happens in ONE place,
// trav_maintain, called at the top of a step for the lanes that need it; the pops and pushes of the step are the plain
// LDS ones.  A lane with entries in the deep store carries T.sb = kDeepSb (-2; its real bottom is row 0 and it gives
// nothing away to idle lanes meanwhile) and is kept at >= 2 LDS entries at the top of every step — a step pops at most
// twice — so its pop test `sp > sb` never fails while the deep store still holds something.  One unsigned compare finds
// both kinds of lane:  (unsigned)(sp + sb) >= limit - 4  (DeviceScene.stack_attn) is true for a lane close to its last rows (sb >= 0; two rows
// early, or earlier for a lane that has given entries away — trav_maintain looks again) and for a flagged lane with
// sp < 2 (sp - 2 wraps) or close to its last rows.  (Tests in the pops themselves cost 2 % of the walk, a deep count
// read from LDS on every empty pop 7 %: profiles/r03_occupancy_ab.log.)
// The pops read LDS and wait for it (up to two round trips per step, on the wave's serial chain between its node
// arithmetic and its request).  Keeping the top row(s) in registers instead was built three ways and measured — a reload
// inside the pop, one row or two rows read again behind every step's request (the last leaves no LDS read and no LDS
// wait on the chain at all): SQ_WAIT_ANY - 3 %, SQ_WAIT_INST_ANY + 2 %, the frame 1.2 - 1.9 % SLOWER each time.  Not
// kept: DESIGN.md section 5 "The stack top in a register", profiles/stack_top_*.
constexpr int kDeepSb = -2;
__device__ __forceinline__ int* trav_deep_count(const DeviceScene& sc, int* stack) { return stack + (size_t)sc.stack_limit * kBlock; }
__device__ __forceinline__ void trav_deep_reset(const DeviceScene& sc, int* stack) {
    if (sc.deep != nullptr) *trav_deep_count(sc, stack) = 0;
}
__device__ __forceinline__ bool trav_needs_maintenance(const DeviceScene& sc, const Trav& T) {
    return (unsigned)(T.sp + T.sb) >= sc.stack_attn;   // stack_limit - 4 with a deep store, else never
}
// (rolled loops: these paths are as good as never taken, their code should stay small inside the traversal loop)
__device__ __forceinline__ void trav_maintain(const DeviceScene& sc, Trav& T, int* stack) {
    if (sc.deep == nullptr) return;   // (without a deep store stack_limit covers the tree's worst case)
    int* cnt = trav_deep_count(sc, stack);
    int32_t* col = sc.deep + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (T.sb < 0) {
        if (T.sp < 2) {   // the newest chunk comes back, below the entry that may be left
            const int have = *cnt;
            if (T.sp == 1) stack[kDeepChunk * kBlock] = stack[0];
#pragma unroll 1
            for (int i = 0; i < kDeepChunk; ++i) stack[i * kBlock] = col[(size_t)(have - kDeepChunk + i) * sc.deep_lanes];
            T.sp += kDeepChunk;
            *cnt = have - kDeepChunk;
            if (have == kDeepChunk) T.sb = 0;
            return;
        }
    } else if (T.sb > 0) {   // close the gap left by donated entries
        const int n = T.sp - T.sb;
#pragma unroll 1
        for (int i = 0; i < n; ++i) stack[i * kBlock] = stack[(T.sb + i) * kBlock];
        T.sb = 0; T.sp = n;
    }
    if (T.sp + 2 >= sc.stack_limit) {   // a node visit writes up to row sp + 2: the oldest chunk goes out
        const int have = *cnt;
#pragma unroll 1
        for (int i = 0; i < kDeepChunk; ++i) col[(size_t)(have + i) * sc.deep_lanes] = stack[i * kBlock];
#pragma unroll 1
        for (int i = kDeepChunk; i < T.sp; ++i) stack[(i - kDeepChunk) * kBlock] = stack[i * kBlock];
        T.sp -= kDeepChunk;
        T.sb = kDeepSb;
        *cnt = have + kDeepChunk;
    }
}
// next pending entry into T.cur (kDone: none left)
__device__ __forceinline__ void trav_pop(const DeviceScene& sc, Trav& T, int* stack) {
    if (T.sp > T.sb) { --T.sp; T.cur = NodeLayout::cursor(stack[T.sp * kBlock]); }
    else T.cur = kDone;
}

__device__ __forceinline__ void trav_settle(const DeviceScene& sc, Trav& T, int* stack) {
    if (T.tri_i >= T.tri_n && T.cur < 0 && T.cur != kDone) {
        NodeLayout::leaf_range(T.cur, T.tri_i, T.tri_n);
        trav_pop(sc, T, stack);
    }
}

// which lanes request what, and where: the statement itself is the layout's (NodeLayout::request)
__device__ __forceinline__ void trav_issue(const DeviceScene& sc, Trav& T, NodeRegs& N, TriRegs& X) {
    // (the compare is made on the register: what the compiler knows of tri_i < tri_n from the branches behind it is a
    // lane mask spread over several scalar registers, which it would turn into 0 / 1 per lane and compare again)
    // (made opaque in place: a copy of tri_i for the compare would be a v_mov on the way to the request)
    asm volatile("" : "+v"(T.tri_i));
    const int ti = T.tri_i;
    const unsigned long long mn = lane_mask(T.cur >= 0), mt = lane_mask(ti < T.tri_n);   // subsets of EXEC
    // (offsets of lanes that want nothing are never dereferenced)
    const uint32_t no = NodeLayout::node_offset(T.cur);
    const uint32_t to = offset48((uint32_t)ti);
    NodeLayout::request(sc, N, X, no, to, mn, mt);
}

__device__ __forceinline__ void trav_wait(NodeRegs& N, TriRegs& X) { NodeLayout::wait(N, X); }
// Before a traversal returns, every record it has requested must have landed: the compiler knows nothing of loads in
// flight and would hand their destination registers to other values (an any-hit query ends with requests outstanding).
__device__ __forceinline__ void trav_drain(NodeRegs& N, TriRegs& X, TriRegs& Y) { NodeLayout::drain(N, X, Y); }

// the triangle that arrived with this step (leaf-order index `tested`): Moeller-Trumbore, closest-hit update as selects
template <bool ANY, bool IGN = false>
__device__ __forceinline__ void trav_tri_part(const Ray& r, Trav& T, const TriRegs& X, const int tested,
                                              uint32_t ignore_object = 0xFFFFFFFFu) {
    const float4 a = make_float4(X.a.x, X.a.y, X.a.z, X.a.w), b = make_float4(X.b.x, X.b.y, X.b.z, X.b.w),
                 c = make_float4(X.c.x, X.c.y, X.c.z, X.c.w);   // triangle: v0 | e1 | e2 (+ material, id, object)
    float t = 0.0f;
    // IGN: FCollisionQueryParams::AddIgnoredActor — triangles of one actor (object id in c.w) are skipped
    bool hit = tri_hit(a, b, c, r, T.t, t);
    if (IGN) hit = hit & (__float_as_uint(c.w) != ignore_object);
    const uint32_t id = __float_as_uint(c.z);
    if (ANY) {
        if (hit) {
            T.t = t; T.leaf_index = tested; T.id = id;
            T.tri_i = 0; T.tri_n = 0; T.cur = kDone; T.sp = 0; T.sb = 0;  // first hit ends the query (records already requested are ignored)
        }
    } else {
        // closest hit, ties to the lower input index — as selects, not branches.  (t, id) compares as ONE 64-bit
        // key: t > 0, so its bits order like an integer, and a traversal without a hit yet carries id = ~0
        // (equivalent to t < T.t | no hit yet | (t == T.t & id < T.id); one v_cmp_lt_u64 instead of five compares)
        const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | id;
        const unsigned long long cur = ((unsigned long long)__float_as_uint(T.t) << 32) | T.id;
        const bool better = hit & (key < cur);
        T.t = better ? t : T.t;
        T.leaf_index = better ? tested : T.leaf_index;
        T.id = better ? id : T.id;
    }
}

// The signs of a ray's direction (of its reciprocals: `inv < 0.0f`, so -0.0 and NaN count as positive) as three lane
// masks of the wave, in scalar registers.  They pick the entry / exit plane words of every node visit; a lane's ray
// changes only when it takes another lane's ray in the sharing round, so the three compares are made where a traversal
// starts and again in a round in which lanes have taken rays (for the whole wave), not once per visit.  Only lanes
// that were active at ray_signs() may use the masks.
struct RaySigns { unsigned long long x, y, z; };
__device__ __forceinline__ RaySigns ray_signs(const Ray& r) {
    return RaySigns{lane_mask(r.ix < 0.0f), lane_mask(r.iy < 0.0f), lane_mask(r.iz < 0.0f)};
}
// m's bit of this lane ? if_set : if_clear, the mask as the select's scalar condition
__device__ __forceinline__ uint32_t lane_select(unsigned long long m, uint32_t if_set, uint32_t if_clear) {
    uint32_t out;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(out) : "v"(if_clear), "v"(if_set), "s"(m));
    return out;
}

// fminf of two canonical values as the bare instruction (the compiler cannot see that the loop-carried bound is
// canonical — trav_init — and would put v_max_f32 t, t in front of every visit's mins)
__device__ __forceinline__ float min_canonical(float a, float b) {
    float out;
    asm("v_min_f32 %0, %1, %2" : "=v"(out) : "v"(a), "v"(b));
    return out;
}

// the lane's inner node (T.cur >= 0): 4 child boxes, near-first order, far children to the stack, next node
__device__ __forceinline__ void trav_node_part(const DeviceScene& sc, const Ray& r, const RaySigns& sg, Trav& T, int* stack,
                                               const NodeRegs& N) {
    // ---- 4-wide node, child boxes on the node's 8-bit grid: plane distance = fma(q, step*inv, (origin-o)*inv)
    const NodeBox n = NodeLayout::decode(N, r);
    const float bx = fmaf(n.ox, r.ix, r.nox);
    const float by = fmaf(n.oy, r.iy, r.noy);
    const float bz = fmaf(n.oz, r.iz, r.noz);
    // the ray's direction signs pick the entry / exit plane words once per node
    const uint32_t nxw = lane_select(sg.x, n.hix, n.lox), fxw = lane_select(sg.x, n.lox, n.hix);
    const uint32_t nyw = lane_select(sg.y, n.hiy, n.loy), fyw = lane_select(sg.y, n.loy, n.hiy);
    const uint32_t nzw = lane_select(sg.z, n.hiz, n.loz), fzw = lane_select(sg.z, n.loz, n.hiz);
    uint32_t key[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // entry and exit plane distances per axis: six plain fmas.  (As three v_pk_fma_f32 — twelve instructions fewer
        // per visit — the frame is 1.4 % slower: a packed f32 operation costs more than the two it replaces and wants
        // its operands in aligned register pairs.  DESIGN.md section 5.)
        const float tnx = fmaf((float)((nxw >> (8 * c)) & 0xFFu), n.sx, bx), tfx = fmaf((float)((fxw >> (8 * c)) & 0xFFu), n.sx, bx);
        const float tny = fmaf((float)((nyw >> (8 * c)) & 0xFFu), n.sy, by), tfy = fmaf((float)((fyw >> (8 * c)) & 0xFFu), n.sy, by);
        const float tnz = fmaf((float)((nzw >> (8 * c)) & 0xFFu), n.sz, bz), tfz = fmaf((float)((fzw >> (8 * c)) & 0xFFu), n.sz, bz);
        const float tn = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, 0.0f));
        const float tf = fminf(fminf(tfx, tfy), min_canonical(tfz, T.t));
        key[c] = tn <= tf ? NodeLayout::hit_key(N, tn, c) : NodeLayout::miss_key(c);
    }
    int ref0, ref1, ref2, ref3;   // the children's references, nearest first
    NodeLayout::order(N, key, ref0, ref1, ref2, ref3);
    constexpr uint32_t kMiss = NodeLayout::kMiss;
    // the number of children hit, read off the sorted keys: at least k + 1 <=> key[k] is a hit
    const bool h1 = key[0] < kMiss, h2 = key[1] < kMiss, h3 = key[2] < kMiss, h4 = key[3] < kMiss;
#ifdef FS_TRAV_STATS
    atomicAdd(&g_trav_stats[5 + (h2 ? 2 : (h1 ? 1 : 0))], 1ull);   // [5] visits with no child hit, [6] one, [7] two or more
#endif
    // far children wait on the stack, farthest pushed first, at sp .. sp + hits - 2: with two hits all three stores
    // land on sp and the last one (the second nearest) stays, with three hits the first two share sp — no store
    // goes above the new top, so the stack needs exactly the tree's worst-case number of rows.  With fewer than two
    // hits the three stores write (unused) words to the free row above the top: cheaper than branching around them,
    // a wave nearly always has a lane that pushes.
    const int p3 = T.sp;
    const int p2 = p3 + (h4 ? 1 : 0);
    const int p1 = p2 + (h3 ? 1 : 0);
    stack[p3 * kBlock] = ref3;
    stack[p2 * kBlock] = ref2;
    stack[p1 * kBlock] = ref1;
    T.sp = p1 + (h2 ? 1 : 0);
    if (h1) T.cur = NodeLayout::cursor(ref0);
    else trav_pop(sc, T, stack);
}

// One whole step of a busy lane, in the pipelined order: node part, advance, request the next records (the
// triangle into `nxt`), then the triangle part on `cur` while they are in flight.  Entry: the records of (T.cur,
// T.tri_i) have arrived in (N, cur).
template <bool ANY, bool IGN = false, bool COUNT = false>
__device__ __forceinline__ void trav_advance(const DeviceScene& sc, const Ray& r, const RaySigns& sg, Trav& T, int* stack, NodeRegs& N,
                                             TriRegs& cur, TriRegs& nxt, uint32_t ignore_object = 0xFFFFFFFFu) {
    const bool has_tri = T.tri_i < T.tri_n;
    const bool has_node = T.cur >= 0;
    const int tested = T.tri_i;
    if (COUNT) { T.nv += has_node ? 1u : 0u; T.nt += has_tri ? 1u : 0u; }
#ifdef FS_TRAV_STATS   // diagnostic build only (tests/trav_stats.py): SIMD occupancy of the two step kinds
    {
        const unsigned long long mt = __ballot(has_tri), mn = __ballot(has_node);
        unsigned long long* gs = g_trav_stats + (ANY ? 16 : 0);
        if ((threadIdx.x & 63u) == (unsigned)(__ffsll((long long)__ballot(true)) - 1)) {
            atomicAdd(&gs[0], 1ull);
            if (mn) { atomicAdd(&gs[1], 1ull); atomicAdd(&gs[2], (unsigned long long)__popcll(mn)); }
            if (mt) { atomicAdd(&gs[3], 1ull); atomicAdd(&gs[4], (unsigned long long)__popcll(mt)); }
            atomicAdd(&gs[11], (unsigned long long)__popcll(mn & mt));
        }
    }
#endif
    // bounded LDS stack: a node visit writes up to row sp + 2.  Checked here, ahead of the node arithmetic and as one
    // scalar branch for the wave, so that the node part stays a single basic block; lanes of trees without a deep store
    // (stack_limit = worst case + 1) may pass the test near their worst case and return at once.
#ifndef FS_DEEP_NO_CHECK   // compiled out in the wide flavour of the frame kernel (worst-case rows, fs_frame.hip)
    if (__builtin_expect(lane_mask(trav_needs_maintenance(sc, T)) != 0ull, 0)) {
        if (trav_needs_maintenance(sc, T)) trav_maintain(sc, T, stack);
    }
#endif
    if (has_node) trav_node_part(sc, r, sg, T, stack, N);
    if (has_tri) ++T.tri_i;
    trav_settle(sc, T, stack);
    if (COUNT) {   // counting instantiation only: how coherent is this wave's node request?  lanes that take part, distinct 64-B records among them
        const unsigned long long mn = __ballot(T.cur >= 0);
        if (mn != 0ull) {
            unsigned distinct = 0;
            for (unsigned long long rest = mn; rest != 0ull; rest &= rest - 1ull) {
                const int l = __ffsll((long long)rest) - 1;
                const int v = __builtin_amdgcn_readlane(T.cur, l);
                const unsigned long long same = __ballot(T.cur == v) & mn;
                distinct += (__ffsll((long long)same) - 1) == l ? 1u : 0u;
            }
            if ((threadIdx.x & 63u) == (unsigned)(__ffsll((long long)__ballot(true)) - 1)) {
                T.ni += 1u; T.nl += (uint32_t)__popcll(mn); T.nd += distinct;
            }
        }
    }
    trav_issue(sc, T, N, nxt);
    // the triangle test must stay BEHIND the requests: it is plain arithmetic on registers, which the compiler would
    // otherwise move in front of the (to it unrelated) load instructions — and then fold the two register sets into one
    asm volatile("" : "+v"(cur.a), "+v"(cur.b), "+v"(cur.c));
    if (has_tri) trav_tri_part<ANY, IGN>(r, T, cur, tested, ignore_object);
}

// one ray per lane without work sharing (tests, tools, diagnostic builds); returns the number of steps taken
template <bool ANY, bool IGN = false>
__device__ __forceinline__ int trav_run(const DeviceScene& sc, const Ray& r, Trav& T, int* stack,
                                        uint32_t ignore_object = 0xFFFFFFFFu) {
    NodeRegs N;
    TriRegs X, Y;
    int steps = 0;
    const RaySigns sg = ray_signs(r);
    trav_settle(sc, T, stack);
    trav_issue(sc, T, N, X);
    // The loop is wave-uniform (lanes whose ray is finished idle along): a per-lane exit would make the compiler carry
    // every lane's register sets out of the loop through copies — of registers that may still be in flight.
    while (true) {
        if (__ballot(trav_busy(T)) == 0ull) break;
        trav_wait(N, X);
        if (trav_busy(T)) { trav_advance<ANY, IGN>(sc, r, sg, T, stack, N, X, Y, ignore_object); ++steps; }
        if (__ballot(trav_busy(T)) == 0ull) break;
        trav_wait(N, Y);
        if (trav_busy(T)) { trav_advance<ANY, IGN>(sc, r, sg, T, stack, N, Y, X, ignore_object); ++steps; }
    }
    trav_drain(N, X, Y);
    return steps;
}

// ImpactNormal: the record's unit geometric normal, flipped to face the ray origin side; material of the hit
__device__ __forceinline__ void hit_surface(const DeviceScene& sc, int leaf_index, const Ray& r, float& nx, float& ny,
                                            float& nz, uint32_t& mat) {
    const float4 c = sc.tris[leaf_index].c;
    const float4 d = sc.tri_nrm[leaf_index];
    float x = d.x, y = d.y, z = d.z;
    float dn = fmaf(x, r.dx, fmaf(y, r.dy, z * r.dz));
    if (dn > 0.0f) { x = -x; y = -y; z = -z; }
    nx = x; ny = y; nz = z;
    mat = __float_as_uint(c.y);
}

// ---------------------------------------------------------------------------------------------------
// Wave work sharing for closest-hit AND any-hit queries (one implementation, three instantiations).
//
// The rays of a wave need very different numbers of traversal steps (median 19, p99 40) and the wave waits for
// its slowest ray in every bounce.  A query parallelises: disjoint subtrees can be searched by different lanes.
// So a lane that has finished its own ray takes the OLDEST pending subtree (bottom of the stack: the one its
// owner would reach last) from a lane that still has pending entries, traverses it with that lane's ray and
// reports into the owner's LDS mailbox.  All of it happens inside one wave (lock-step), without atomics on the stacks.
//   closest hit (ANY = false): the partial answers merge by atomicMin on the 64-bit key (t bits << 32 | triangle
//     id) — exactly the (t, id) order a single traversal applies, so the result does not depend on who searched
//     what; a taken subtree starts from min(donor's bound, owner's mailbox).
//   any hit (ANY = true): most connection rays are blocked and end at their first hit, the unobstructed ones must
//     search every box along the segment; a hit anywhere settles the ray (flag in the owner's mailbox) and lanes
//     still searching for a settled ray drop their work.
//   IGN: FCollisionQueryParams::AddIgnoredActor per ray (legacy tracer).
// LDS rows of kBlock words: rays (closest: origin, direction, reciprocals = 9 rows, the thief recomputes -o*inv;
// any: origin, direction, tmax = 7 rows — the thief recomputes the reciprocals too, 40 B per lane keep two connect
// workgroups on a CU next to the histogram) | [ignored actor] | mailbox (closest: u64 key + leaf; any: blocked flag) | donation boxes ref,
// owner [, bound].  Every lane of the wave must call it (has_ray = false: nothing of its own, helps from the start).
// ---------------------------------------------------------------------------------------------------
template <bool ANY, bool IGN>
struct ShareArea {
    static constexpr int kRayRows = ANY ? 7 : 9;
    static constexpr int kRows = kRayRows + (IGN ? 1 : 0) + (ANY ? 1 : 3) + 2 + (ANY ? 0 : 1);
    static constexpr size_t kBytes = (size_t)kBlock * 4 * kRows;
    float* rs; uint32_t* rign; unsigned long long* rkey; int* rleaf; int* blocked; int* dref; int* down; float* dbound;
    __device__ __forceinline__ explicit ShareArea(int* base) {
        rs = reinterpret_cast<float*>(base);
        int* p = base + kRayRows * kBlock;
        rign = reinterpret_cast<uint32_t*>(p); if (IGN) p += kBlock;
        rkey = reinterpret_cast<unsigned long long*>(p); blocked = p; rleaf = p + 2 * kBlock;
        p += (ANY ? 1 : 3) * kBlock;
        dref = p; down = p + kBlock; dbound = reinterpret_cast<float*>(p + 2 * kBlock);
    }
};
constexpr size_t kShareLdsBytes = ShareArea<false, false>::kBytes;      // 60 B per lane
// The sharing round (ballots, donation boxes, the thieves' ray reload: ~50 VALU + ~35 SALU for the whole wave) runs only
// once this many lanes have nothing to do: feeding the first few idle lanes costs every lane more than it returns.
// Measured at cfg3 (profiles/r02_share_min_idle.log): 1 / 4 / 8 / 16 / 24 / 32 / 48 -> walk 0.304 / 0.303 / 0.298 /
// 0.294 / 0.300 / 0.309 / 0.334 ms, connect 0.075 -> 0.072 ms at 16.  Sparse waves start above it.
// (again on round 5's fused stream, profiles/r05_share_min_idle.log: 8 / 12 / 16 / 20 / 24 -> 971 / 981 / 988 / 981 / 975 M rays/s.)
constexpr int kShareMinIdle = 16;
constexpr size_t kShareAnyLdsBytes = ShareArea<true, false>::kBytes;    // 40 B per lane
constexpr size_t kShareIgnLdsBytes = ShareArea<false, true>::kBytes;    // 64 B per lane

// returns: ANY — the ray is blocked; closest — a hit was found (T.t, T.id, T.leaf_index describe it)
template <bool ANY, bool IGN, bool COUNT = false>
__device__ __forceinline__ bool trav_shared(const DeviceScene& sc, bool has_ray, const Ray& own, float tmax,
                                            uint32_t ignore, Trav& T, int* stack, int* share) {
    const ShareArea<ANY, IGN> A(share);
    float* rs = A.rs;
    const unsigned tid = threadIdx.x, wbase = tid & ~63u;
    // publish this lane's ray and clear its mailbox
    rs[0 * kBlock + tid] = own.ox;  rs[1 * kBlock + tid] = own.oy;  rs[2 * kBlock + tid] = own.oz;
    rs[3 * kBlock + tid] = own.dx;  rs[4 * kBlock + tid] = own.dy;  rs[5 * kBlock + tid] = own.dz;
    if (ANY) {
        rs[6 * kBlock + tid] = tmax;
        A.blocked[tid] = 0;
    } else {
        rs[6 * kBlock + tid] = own.ix;  rs[7 * kBlock + tid] = own.iy;  rs[8 * kBlock + tid] = own.iz;
        A.rkey[tid] = ~0ull;
        A.rleaf[tid] = -1;
    }
    if (IGN) A.rign[tid] = ignore;
    unsigned owner = tid;   // block-local lane whose ray this lane is working on
    uint32_t wign = ignore;
    Ray wr = own;
    RaySigns sg = ray_signs(wr);   // of the rays the lanes work on: made again below when lanes have taken others
    trav_init(T, tmax, has_ray && sc.num_nodes > 0);
    trav_deep_reset(sc, stack);
    // The records of the NEXT step are requested as soon as this step has decided what they are: behind the node part
    // of the step, before its triangle test (trav_advance) and before the work-sharing round below (ballots, donation
    // boxes, mailboxes: half a dozen LDS round trips), which both run in the shadow of the fetch.  A wave in the thin
    // tail of the frame runs alone on its SIMD and nothing else hides that latency.  Lanes that take work in the round
    // request theirs at its end.  The triangle records alternate between two register sets (the loop body is
    // instantiated twice): the one being tested is still needed while the next one is already arriving.
    NodeRegs N;
    TriRegs X, Y;
    trav_settle(sc, T, stack);
    trav_issue(sc, T, N, X);
    // one step of the wave; cur = the triangle registers that arrive with this step, nxt = the ones requested for the
    // next.  true = nothing is left anywhere in the wave.
    auto step = [&](TriRegs& cur, TriRegs& nxt) -> bool {
        trav_wait(N, cur);
#ifdef FS_TRAV_STATS
        {
            const unsigned long long mb = __ballot(trav_busy(T)), mth = __ballot(trav_busy(T) && owner != tid);
            if ((tid & 63u) == 0u) {
                unsigned long long* gs = g_trav_stats + (ANY ? 16 : 0);
                atomicAdd(&gs[8], (unsigned long long)__popcll(mb)); atomicAdd(&gs[9], (unsigned long long)__popcll(mth));
                atomicAdd(&gs[10], 1ull);
            }
        }
#endif
        if (trav_busy(T)) {
            trav_advance<ANY, IGN, COUNT>(sc, wr, sg, T, stack, N, cur, nxt, wign);
            if (ANY) {
                if (T.leaf_index >= 0) { A.blocked[owner] = 1; T.leaf_index = -1; }   // first hit ends the query (T is idle now)
                else if (A.blocked[owner]) { T.cur = kDone; T.sp = 0; T.sb = 0; T.tri_i = 0; T.tri_n = 0; }   // settled by another lane
            } else if (!trav_busy(T) && T.leaf_index >= 0) {   // this (sub)traversal is over: report to the owner of the ray
                const unsigned long long key = ((unsigned long long)__float_as_uint(T.t) << 32) | (unsigned long long)T.id;
                atomicMin(&A.rkey[owner], key);
                if (A.rkey[owner] == key) A.rleaf[owner] = T.leaf_index;
            }
        }
        const bool idle = !trav_busy(T);
        // (one ballot per compare, joined as scalars)
        const unsigned long long busy_m = lane_mask(T.tri_i < T.tri_n) | lane_mask(T.cur != kDone);
        if (busy_m == 0ull) return true;                // nothing left anywhere in the wave
        const unsigned long long idle_m = lane_mask(true) & ~busy_m;   // (the lanes here that are not busy: no second ballot)
        if (__popcll(idle_m) < kShareMinIdle) return false;
        const bool can_give = !idle && T.sp > T.sb && T.sb >= 0;   // (a lane with entries in the deep store keeps what it has)
        const unsigned long long give_m = lane_mask(can_give);
        if (idle_m != 0ull && give_m != 0ull) {
            const int n = min(__popcll(idle_m), __popcll(give_m));
            if (can_give) {
                const int r = lanes_below(give_m);
                if (r < n) {
                    A.dref[wbase + r] = stack[T.sb * kBlock];
                    A.down[wbase + r] = (int)owner;
                    if (!ANY) A.dbound[wbase + r] = T.t;
                    ++T.sb;
                    if (T.sb == T.sp) { T.sb = 0; T.sp = 0; }
                }
            }
            if (idle) {
                const int r = lanes_below(idle_m);
                if (r < n) {
                    const int e = A.dref[wbase + r];
                    owner = (unsigned)A.down[wbase + r];
                    float bound;
                    if (ANY) {
                        wr = make_ray(rs[0 * kBlock + owner], rs[1 * kBlock + owner], rs[2 * kBlock + owner],
                                      rs[3 * kBlock + owner], rs[4 * kBlock + owner], rs[5 * kBlock + owner]);
                        bound = rs[6 * kBlock + owner];
                    } else {
                        // the owner's mailbox may already hold a closer hit than the donor knew of
                        bound = __uint_as_float(min(__float_as_uint(A.dbound[wbase + r]), (uint32_t)(A.rkey[owner] >> 32)));
                        wr.ox = rs[0 * kBlock + owner];  wr.oy = rs[1 * kBlock + owner];  wr.oz = rs[2 * kBlock + owner];
                        wr.dx = rs[3 * kBlock + owner];  wr.dy = rs[4 * kBlock + owner];  wr.dz = rs[5 * kBlock + owner];
                        wr.ix = rs[6 * kBlock + owner];  wr.iy = rs[7 * kBlock + owner];  wr.iz = rs[8 * kBlock + owner];
                        wr.nox = -(wr.ox * wr.ix); wr.noy = -(wr.oy * wr.iy); wr.noz = -(wr.oz * wr.iz);   // as make_ray
                    }
                    if (IGN) wign = A.rign[owner];
                    T.cur = NodeLayout::cursor(e); T.sp = 0; T.sb = 0; T.tri_i = 0; T.tri_n = 0;
                    T.t = canonical_bound(bound); T.leaf_index = -1; T.id = 0xFFFFFFFFu;
                    trav_deep_reset(sc, stack);   // (an any-hit query that ended early may have left entries there)
                    trav_settle(sc, T, stack);
                    trav_issue(sc, T, N, nxt);
                }
            }
            sg = ray_signs(wr);   // (n >= 1 here: some lane has taken a ray; every lane of the wave is back at this point)
        }
        return false;
    };
    while (true) {
        if (step(X, Y)) break;
        if (step(Y, X)) break;
    }
    trav_drain(N, X, Y);
    if (ANY) return A.blocked[tid] != 0;
    // everything searched: the mailbox holds the closest hit of this lane's own ray
    const unsigned long long key = A.rkey[tid];
    if (key != ~0ull) {
        T.t = __uint_as_float((uint32_t)(key >> 32));
        T.id = (uint32_t)key;
        T.leaf_index = A.rleaf[tid];
        return true;
    }
    T.t = tmax;
    T.leaf_index = -1;
    T.id = 0xFFFFFFFFu;
    return false;
}
// the three uses: BDPT walk, ConnectSubpaths' visibility ray, legacy tracer
template <bool COUNT = false, bool IGN = false>
__device__ __forceinline__ void trav_run_shared(const DeviceScene& sc, const Ray& own, Trav& T, int* stack, int* s_dyn,
                                                float tmax, bool has_ray = true, uint32_t ignore = 0xFFFFFFFFu) {
    trav_shared<false, IGN, COUNT>(sc, has_ray, own, tmax, ignore, T, stack, s_dyn + (size_t)sc.stack_rows * kBlock);
}
template <bool COUNT = false>
__device__ __forceinline__ bool trav_any_shared(const DeviceScene& sc, bool has_ray, const Ray& own, float tmax,
                                                int* stack, int* share, uint32_t* nv = nullptr, uint32_t* nt = nullptr) {
    Trav T;
    const bool blocked = trav_shared<true, false, COUNT>(sc, has_ray, own, tmax, 0xFFFFFFFFu, T, stack, share);
    if (COUNT) { *nv += T.nv; *nt += T.nt; }
    return blocked;
}
// COUNT instantiations: this lane's record fetches -> the frame scratch's work counters (one atomic per lane: the
// counting frames are not timed)
__device__ __forceinline__ void add_fetch_counts(unsigned* scratch, int first_counter, uint32_t nv, uint32_t nt) {
    unsigned long long* counters = reinterpret_cast<unsigned long long*>(scratch + kCounterWord);
    if (nv) atomicAdd(&counters[first_counter], (unsigned long long)nv);
    if (nt) atomicAdd(&counters[first_counter + 1], (unsigned long long)nt);
}

}  // namespace
}  // namespace fs
