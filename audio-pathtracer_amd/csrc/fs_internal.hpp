// fs_internal.hpp — internal types shared by the host library and the HIP kernels (gfx950).
// Not part of the public boundary (that is include/frequensee.h).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/frequensee.h"

#if defined(FS_TRAV_STATS) && !defined(FS_EXPERIMENTS)
#define FS_EXPERIMENTS   // the traversal statistics are recorded by the one-subpath-per-lane walk kernel
#endif

namespace fs {

// ---- device data layout (HBM) --------------------------------------------------------------------
// 4-wide BVH node, 64 B = half a 128-B cache line = four 16-byte loads:
//   q0 = (origin.x origin.y origin.z, step.x)  step: the power-of-two grid step of each axis, as a float (the
//                                             traversal multiplies it by the ray's reciprocal direction right away)
//   q1 = (lox4 loy4 loz4 hix4)  q2 = (hiy4 hiz4 step.y step.z)   byte c of each word = child c's plane on that
//                                             grid: box = origin + q * step, rounded outwards
//   q3 = child[4] as int bits; child >= 0: inner node index; child < 0: leaf,
//        ~child = first_tri * 4 + (count - 1), count in 1..4 (the builder makes 1..2); empty slot: lo = 255 > hi = 0 (never hit).
struct alignas(16) NodeQ4 {
    float ox, oy, oz;
    float sx;
    uint32_t lox, loy, loz, hix;
    uint32_t hiy, hiz;
    float sy, sz;
    int32_t child[4];
};
static_assert(sizeof(NodeQ4) == 64, "NodeQ4 must be 64 B");

// Triangle record, 64 B (the intersection test reads the first 48 B, the hit shading the last 16 B),
// stored in leaf order:
//   a = (v0.x v0.y v0.z e1.x)  b = (e1.y e1.z e2.x e2.y)  c = (e2.z, material, input index, object id)
//   d = (unit geometric normal of cross(e1, e2), -)
struct alignas(16) Tri64 {
    float4 a, b, c, d;
};
static_assert(sizeof(Tri64) == 64, "Tri64 must be 64 B");

// What the kernels read: the first 48 B of every Tri64 at a 48-B stride (the intersection test never sees the normal:
// without it the records the traversal keeps pulling through L1/L2 take a quarter less room) and the unit normals in
// an array of their own (read once per walk step, at the hit).  Tri64 stays the authoring format of the builders, the
// refit and fs_scene_update_triangles; launch_pack_triangles / update_tris_kernel derive the kernels' view from it.
struct alignas(16) Tri48 {
    float4 a, b, c;
};
static_assert(sizeof(Tri48) == 48, "Tri48 must be 48 B");

// What the cooperative traversal of small frames reads (fs_dev_coop.hpp: trav_coop): one 16-byte record per CHILD — a lane
// tests one child box per step and fetches exactly its own record, with one ds_read_b128 (the first DeviceScene.lds_nodes
// nodes of the breadth-first array are staged in LDS by every workgroup) or one global_load_dwordx4 — derived from the
// NodeQ4 array after every commit and refit (fs_refit.hip: coop_nodes_kernel):
//   lo.x lo.y | lo.z hi.x | hi.y hi.z   the child's box as fp16, rounded outwards (conservative; an empty slot is the
//                                       inverted box +inf / -inf), ref = NodeQ4.child[c]
// Record 4 * node + child (an intermediate array), then folded TWO LEVELS AT A TIME into 16-wide nodes — record
// 16 * dense node + slot, 256 B per node, inner references = dense indices of the even levels (fs_refit.hip:
// coop16_kernel): a query takes half as many steps.  DeviceScene.coop points at the 16-wide array.
struct alignas(16) CoopChild {
    uint32_t lo_xy, loz_hix, hi_yz;
    int32_t ref;
};
static_assert(sizeof(CoopChild) == 16, "CoopChild must be 16 B");

// What a cooperative kernel is given beside the scene: one of the two node arrays of that traversal.
//   wshift 4: the 16-wide nodes (two levels of the 4-wide tree folded together, dense order of the even levels): half the
//             steps per query — what waves of one or two rays walk (a group of 64 / 32 lanes takes 4 / 2 nodes per step);
//   wshift 2: the per-child records of the 4-wide nodes as they are — what waves of FOUR rays walk: a group of 16 lanes
//             takes four of those nodes per step but only one 16-wide one (old_mine, 128 sources: 1.76 against 1.99 ms per tick).
// lds_nodes: nodes [0, lds_nodes) are resident in the workgroup's LDS (set by the launcher: what fits).
// stack_need: worst-case pending entries of a one-node-at-a-time descent (what trav_coop keeps free before it widens).
struct CoopView {
    const CoopChild* rec;     // [nodes << wshift]
    int32_t lds_nodes, nodes;
    int16_t wshift, stack_need;
};
// The chip-filling flavour of the fused frame kernel walks a derived VIEW of the tree instead (fs_refit.hip: the view
// kernels; fs_dev_trav.hpp: NodeLayoutView): inner nodes and triangle records together in ONE array of 48-byte records, every
// node's children — its inner children's node records and each leaf child's 1 - 4 triangle records, in slot order — one
// consecutive block, the root record 0.  A node record is three 16-byte quarters,
//   q0 = (origin.x, origin.y, origin.z, lox)   q1 = (loy, loz, hix, hiy)   q2 = (hiz, G, cb8, E)
// the six plane words of its NodeQ4 verbatim; E = one exponent byte per grid step (x | y << 8 | z << 16), cb8 = the reference
// base of the child block, G = one slot byte per child; the words' formats are the view_* helpers below and nowhere else.
// The normals of the triangle records lie in a parallel float4 array indexed by record number (node slots unused).  Rebuilt
// on the device behind every commit and refit like CoopChild; NodeQ4 / Tri48 stay the tree format of everything else.
struct alignas(16) ViewRec {
    float4 q0, q1, q2;
};
static_assert(sizeof(ViewRec) == sizeof(Tri48), "the view holds node and triangle records at one stride");
// The size rule of the view: the request carries record x 48 as a 32-bit byte offset, and a reference must stay below 2^30
// (the cursor keeps the leaf bit in the sign after the turn by kViewTurn).
constexpr bool node_view_fits(uint64_t nodes, uint64_t tris) {
    return (nodes + tris) * sizeof(ViewRec) <= 0xFFFFFFFFull && nodes + tris <= (1ull << 27);
}
// The view's word formats (the builder, fs_refit.hip: view_nodes_kernel, and the step, fs_dev_trav.hpp: NodeLayoutView, both
// use these; tests/tree_check.py restates them independently).
//   slot byte (byte c of G)   8 x (the slot's first record relative to the child block, <= 12) + 4 x leaf + (triangles - 1)
//   reference                 cb8 + the slot byte = record number x 8 | leaf bit | count - 1, where cb8 = 8 x the block's first record
//   cursor (Trav::cur)        the reference turned right by 3: leaf bit 31 | count - 1 at 30:29 | record number — inner or
//                             leaf is the sign, as it is for a NodeQ4 child
//   exponent byte             bits 30:23 of a grid step, a positive normal power of two: as_float(byte << 23) is the step bit for bit
constexpr uint32_t kViewTurn = 3, kViewLeaf = 1u << (kViewTurn - 1), kViewRecordBits = 32 - kViewTurn;
constexpr uint32_t view_slot_byte(uint32_t offset, bool leaf, uint32_t count) {
    return (offset << kViewTurn) + (leaf ? kViewLeaf + (count - 1u) : 0u);
}
constexpr uint32_t view_ref_base(uint32_t first_record) { return first_record << kViewTurn; }
constexpr uint32_t view_ref(uint32_t cb8, uint32_t slot_byte) { return cb8 + slot_byte; }
constexpr int32_t view_cursor(uint32_t ref) { return (int32_t)((ref >> kViewTurn) | (ref << kViewRecordBits)); }   // (one v_alignbit_b32)
constexpr bool view_is_leaf(int32_t cur) { return cur < 0; }
constexpr int32_t view_record(int32_t cur) { return cur & (int32_t)((1u << kViewRecordBits) - 1u); }
constexpr int32_t view_count(int32_t cur) { return ((cur >> kViewRecordBits) & (int32_t)(kViewLeaf - 1u)) + 1; }
constexpr uint32_t view_exp_byte(uint32_t step_bits) { return (step_bits >> 23) & 0xFFu; }
constexpr uint32_t view_step_bits(uint32_t exp_byte) { return exp_byte << 23; }
constexpr bool view_round_trip(uint32_t block, uint32_t offset, bool leaf, uint32_t count) {
    const int32_t cur = view_cursor(view_ref(view_ref_base(block), view_slot_byte(offset, leaf, count)));
    return view_is_leaf(cur) == leaf && view_record(cur) == (int32_t)(block + offset) && (!leaf || view_count(cur) == (int32_t)count);
}
static_assert(view_round_trip(0, 0, false, 1) && view_round_trip(0, 0, true, 1) && view_round_trip(0, 12, true, 4) &&
              view_round_trip((1u << 27) - 13, 12, false, 1) && view_round_trip((1u << 27) - 1, 0, true, 4) &&
              view_round_trip((1u << 27) - 13, 12, true, 1), "reference -> cursor at records 0 and 2^27 - 1, counts 1 and 4, offsets 0 and 12");
static_assert(view_slot_byte(12, true, 4) <= 0xFFu, "a slot byte is a byte");
static_assert(!node_view_fits((1u << 27) + 1, 0) && !node_view_fits(0, (1u << 27) + 1) &&
              view_ref(view_ref_base((1u << 27) - 1), view_slot_byte(0, true, 4)) < (1u << 30),
              "node_view_fits admits no record past 2^27 - 1, and the largest reference to that one stays below 2^30");
static_assert(view_step_bits(view_exp_byte(0x3F800000u)) == 0x3F800000u && view_step_bits(view_exp_byte(0x00800000u)) == 0x00800000u &&
              view_step_bits(view_exp_byte(0x7F000000u)) == 0x7F000000u, "a power-of-two step comes back from its exponent byte");
struct NodeView {           // host bookkeeping; rec == null: the scene has no view (too large, a step that is no power of two)
    const ViewRec* rec = nullptr;      // [nodes + triangles]
    const float4* nrm = nullptr;       // [nodes + triangles]
};
struct CoopInfo { CoopView wide16{}, wide4{}; NodeView view{}; };
constexpr float kCoopMaxCoordinate = 16384.0f;   // largest |coordinate| (UE units) of a scene whose small frames use the cooperative traversal (fp16 ulp 8 there)

// Per-lane traversal stack in LDS: DeviceScene.stack_rows rows of kBlock ints, sized at run time from the committed
// tree (its worst-case need + kStackSlack), passed as dynamic shared memory.  A node visit that pushes writes its
// three candidate entries at sp .. sp + hits - 2 — never above the new top — so the worst-case need itself would do;
// one spare row is kept.  LDS size matters beyond occupancy: the walk workgroups of frame f+1 share the CUs with the
// reconstruct workgroups of frame f (tail stream, 4 KB of LDS each), and 3 x walk + 1 x reconstruct must fit the CU's
// 160 KB or the third walk workgroup waits (measured: 52 224 B of dynamic LDS 0.356 ms, 51 200 B 0.315 ms).
constexpr int kStackDepth = 64;   // largest worst-case stack need the builder accepts before it rebuilds shallower
constexpr int kStackSlack = 1;
constexpr int kBlock = 256;       // 4 waves of 64 lanes
// Reconstruct (fs_dev_recon.hpp): a thread filters kChunk consecutive samples, a workgroup one block of kReconBlockSamples.
// A zero-block mask word of a host ring slot has one bit per such block (host_block_vote; the host: slot_masks_usable).
constexpr int kChunk = 16;
constexpr int kReconBlockSamples = kBlock * kChunk;   // 4 096
constexpr int kWarm = 96;                             // samples of filter run-in before a thread's own chunk
// LDS of one reconstruct workgroup: the row's amplitudes [num_bins] | the block's interpolated samples and their run-in
// [kReconBlockSamples + kWarm] | the staged outputs [kBlock][kChunk + 1] (reconstruct_body_fast's layout, also that of the spectral
// row).  fast = false: reconstruct_body's layout (the fused frame's plain rows), which has no interpolated samples.
// fs_context_create refuses a shape whose reconstruct needs more than the device gives one workgroup.
constexpr size_t recon_lds_bytes(int num_bins, bool fast = true) {
    return sizeof(float) * ((size_t)num_bins + (fast ? (size_t)kReconBlockSamples + kWarm : 0) + (size_t)kBlock * (kChunk + 1));
}
// The same two phases in the narrow fused frame kernels (reconstruct_body_staged, and the spectral row everywhere): the amplitudes
// [num_bins] | ONE area that first holds the interpolated samples, a pad word behind every kChunk of them (recon_x_pos), and then
// — the filter's outputs having waited in registers behind a barrier — the staged outputs
constexpr size_t frame_recon_lds_bytes(int num_bins) {
    const size_t x = (size_t)kReconBlockSamples + kWarm, x_padded = x + x / kChunk, stage = (size_t)kBlock * (kChunk + 1);
    return sizeof(float) * ((size_t)num_bins + (x_padded > stage ? x_padded : stage));
}
static_assert(frame_recon_lds_bytes(0) <= recon_lds_bytes(0), "the spectral row of the reconstruct-only kernels runs in recon_lds_bytes");
static_assert(frame_recon_lds_bytes(0) >= recon_lds_bytes(0, false), "a narrow fused launch of one frame runs reconstruct_body in the same LDS");
// Room left next to it for the static LDS of the kernels that run a reconstruct (the fused frame kernels: 1 888 B on gfx950; the
// batch kernel: 256 B for its workgroup vote).  A workgroup's static and dynamic LDS together must fit the device's limit.
constexpr size_t kReconStaticLdsReserve = 4096;
// the most bins whose reconstruct fits `lds` bytes per workgroup
constexpr int max_recon_bins(size_t lds) {
    return lds > recon_lds_bytes(0) + kReconStaticLdsReserve ? (int)((lds - recon_lds_bytes(0) - kReconStaticLdsReserve) / sizeof(float)) : 0;
}
static_assert(64 % kChunk == 0, "carrier_stride (below) must hold whole chunks");
// LDS-privatised part of the [bands][bins] energy histogram in the connect kernels.  With the reference's distance
// scale (cm / 1000, ARTS.cpp:373) bin = path length in metres / 3.43: 256 bins cover 878 m, and a 262 144-ray frame
// at cfg3 touches bins 0..60.  All 1000 bins cost 32 KB per workgroup at 8 bands — the 8 KB window keeps three
// connect workgroups on a CU instead of two.  FS_HIST_WINDOW overrides it (1 .. 4 096, read at fs_context_create;
// tests/test_config_shapes.py: test_hist_window_override runs 1, 16 and 4 096 against the oracle).
constexpr int kHistWindow = 256;
constexpr int kUnboundedDepth = 1 << 24;   // the weights' depth cap when the walk has none: every strategy exists
constexpr int kOverLevels = 448;            // second-tier walk steps of depth = 0 frames (64 + 448 = 512 steps)

// The traversal addresses `nodes` and `tris` by a scalar base and a 32-bit byte offset per lane (fs_dev_trav.hpp:
// trav_issue): num_nodes * sizeof(NodeQ4) and num_tris * sizeof(Tri48) fit 32 bits — a larger scene is refused at commit
// (fs_capi_scene.cpp: finish_commit).  What the three record arrays hold is the business of the kernel's node layout
// (fs_dev_trav.hpp: NodeLayout): a launcher whose unit walks the 48-byte view binds its copy of the scene to the view's
// arrays (NodeLayoutView::bind: nodes == tris == the ViewRec array, tri_nrm the view's normals); nobody else touches them.
struct DeviceScene {
    const NodeQ4* nodes;
    const Tri48* tris;        // traversal records, leaf order
    const float4* tri_nrm;    // unit geometric normals, leaf order
    const float* absorption;  // [M][B]
    const float* lobe_gain;   // [M][3][B] diffuse / specular / transmitted gains (FS_FLAG_MATERIAL_LOBES)
    const float* lobe_prob;   // [M][3] probability of each lobe
    int32_t num_nodes;        // 0 = empty scene
    int32_t num_tris;
    int32_t num_materials;
    int32_t stack_rows;       // LDS rows of the traversal stack area per lane (see kStackDepth); with a deep store the last
                              //   one holds the lanes' deep counts
    int32_t stack_limit;      // rows a lane's pending entries may use in LDS: stack_rows without a deep store (the tree's
                              //   worst case + 1, nothing can overflow), else kStackRowsCap (more goes to `deep`)
    // Deep store (only for trees whose worst case exceeds kStackRowsCap rows): [deep_rows][deep_lanes] ints in HBM, column
    // blockIdx.x * kBlock + threadIdx.x.  A lane whose LDS rows are full moves its oldest entries there in chunks and
    // takes them back when its LDS rows run low (fs_dev_trav.hpp: trav_maintain).  The worst case assumes
    // that a ray hits every child box at every level of the deepest path; rays that need more than kStackRowsCap rows
    // are rare enough that the trips to HBM do not show, and the bounded LDS stack lets four workgroups share a CU.
    uint32_t stack_attn;      // stack_limit - 4 with a deep store, else 0x7FFFFFFF: (unsigned)(sp + sb) >= stack_attn sends a
                              //   lane to trav_maintain at the top of a step (fs_dev_trav.hpp)
    int32_t stack_worst;      // rows of a stack that cannot overflow (worst case + 1) if a workgroup may have that much LDS, else
                              //   0: what the wide flavour of the frame kernel runs with (fs_frame.hip)
    const struct CoopInfo* coop_info;   // host bookkeeping: the cooperative traversal's node arrays (CoopView above) and the 48-byte node view; unused on the device
    int32_t* deep;
    uint32_t deep_lanes;
    struct DeepStore* deep_owner;   // host bookkeeping (grows the store when a launch has more lanes); unused on the device
};

// per-update constants handed to the kernels by value
struct KParams {
    uint32_t seed_lo, seed_hi;
    uint32_t pair_begin;   // first global pair index of this rank
    uint32_t num_local;    // pairs traced by this rank (all sources of a batched frame together)
    uint32_t pairs_per_source;   // == num_local for one source; a batched frame lays its sources' pairs end to end:
                                 // pair li belongs to source li / pairs_per_source, RNG pair index li % pairs_per_source
    const float* src_table;      // [sources][4] source positions (+ the source's actor id as bits) of a batched frame (device), else null (kp.src)
    uint32_t src_object, lis_object;   // the actors the walks ignore (fs_source_set_object / fs_listener_set_object), FS_NO_OBJECT: none
    uint32_t item_seed[4];       // grouped frames (fs_set_frames_per_launch): the low seed word of each item of the batched
    int32_t item_seeds;          //   frame (item_seeds of them; 0 = every item uses seed_lo, the batch of one call)
    int32_t depth;         // max segments per subpath: 1..FS_MAX_DEPTH, or main_levels + over_levels for depth = 0 (a bound the
                           //   roulette practically never reaches: 0.9^512 ~ 4e-24)
    int32_t mis_depth;     // depth cap D of the all-connections weights (kUnboundedDepth for depth = 0)
    int16_t russian_roulette;
    int16_t cosine;
    int16_t ignore_on;     // some walk of the frame ignores an actor: the EXT instantiations run (16 bits each: the fused launch's 4 KB of arguments are full)
    int32_t lobes;         // 1 = FS_FLAG_MATERIAL_LOBES: the walk picks a specular / diffuse / transmitted lobe per vertex
    int16_t mis;           // all-connections mode: 1 = balance-heuristic weights, 0 = uniform
    int16_t plan_coop;     // the plan pass evaluates 64 bounces of a subpath at once, a wave per 8 subpaths (plan_coop_body): frames of <= 32 768 subpaths, and uncapped walks
                           //   that are waited for (the host decides: frame_describe)
    float rr_prob, max_trace_dist, surface_offset, connect_pullback;
    float stage_margin;    // staged walks: lanes a later stage is given = stage_margin x the expected survivors + 1024 (1.3; doubled
                           //   by the overflow retry if a frame ever had more)
    float dist_divisor, min_seg, prob_exponent, energy_clamp, energy_gain, sound_speed;
    float norm;            // 1/P or 1/1000 (ARTS.cpp:164)
    float air[FS_MAX_BANDS];
    float src[3], lis[3];
    int32_t dpos;          // 1 = FS_FLAG_DOUBLE_POSITIONS: node positions, segment and connection lengths in double
    float listener_radius, source_radius;   // collision spheres of the end points, 0 = points
    int32_t count;         // 1 = COUNT instantiations: the kernels also count the records they fetch (fs_set_profiling level 3)
    int32_t num_bins;
    int32_t num_bands;     // bands of the context (the connect kernels are instantiated for 1, 4 and 8; any other count reads this)
    int32_t hist_window;   // the connect kernels privatise bins [0, hist_window) of every band in LDS; deposits beyond go
                           // straight to the energy buffer with global atomics (kHistWindow, or all bins if fewer)
};

constexpr uint32_t kPlanCoopMax = 32768, kPlanCoopMaxUncapped = 1u << 17;   // KParams.plan_coop (fs_dev_walk.hpp: plan_coop_body)

// Source directivity (fs_source_set_directivity): a kernel argument of the directional connect kernels only — KParams,
// ten times in the fused frame kernel's 4 KB of arguments, does not grow.  table == null: omnidirectional (factor 1).
// The same descriptor carries the source's order window (fs_source_set_order_window): a deposit whose path has fewer than
// min_order or more than max_order nodes made by a hit is dropped.  (0, FS_ORDER_UNBOUNDED): no window.
struct Directivity {
    float fwd[3];            // unit forward vector
    int32_t samples;         // K: samples per band
    const float* table;      // device [bands][K], or null
    int32_t min_order = 0, max_order = 0x7fffffff;   // order window, both ends included
};
struct DirArgs {
    Directivity one;         // the frame's source
    const Directivity* tab;  // batched frame: [sources] descriptors (device, in the batch table), indexed li / pairs_per_source; else null
};

// legacy forward tracer (UpdateSound) constants and device-side accumulators
struct SoundKParams {
    uint32_t seed_lo, seed_hi;
    int32_t raycasts_per_tick, raycast_bounces;
    float raycast_distance, simulated_duration, listener_radius;
    float src[3], lis[3];
};
struct SoundAccum {
    unsigned long long traces;
    unsigned reaching, direct_hits;
    float direct_energy_sum, occlusion;
};

// What the walk kernels leave for connect_kernel.  A subpath is known by its index g (side-major: [0,n) source side,
// [n,2n) listener side) and by its LAUNCH SLOT: the lane that walks it under the length-sorted schedule.  Everything
// the walk writes is indexed by slot — a wave's lanes write consecutive words — and slot_of[g] leads back to it
// (null = no schedule, slot == g).  total = 2 * num_local.
struct SubpathState {
    float4* end_pos;    // [total] by slot: xyz = last node position, w = last node probability
    uint2* end_misc;    // [total] by slot: x = last node material, y = segments taken
    float2* seg_np;     // [main_levels][total] per walk step, by slot: x = scaled segment length, y = probability of the
                        //   node EvaluatePath pairs with the segment (departure node on the source side, arrival node
                        //   on the listener side)
    uint32_t* seg_mat;  // [main_levels][total] material of that node
    float4* seg_pos;    // [main_levels][total] xyz = position of the node a walk step arrives at; only written (and only
                        //   non-null) in all-connections mode, which connects interior nodes too (row f3)
    float4* seg_nrm;    // [main_levels][total] xyz = normal of that node; only with balance-heuristic weights
    uint32_t* slot_of;  // [total] launch slot of subpath g, written by the walk; null: slot == g
    // Walk steps beyond main_levels exist only for depth = 0 (no cap, ARTS.cpp:294): 0.9^64 of the walks take more than
    // 64 steps, and the schedule puts the longest walks into the lowest slots, so their later records live in a small
    // second tier [over_levels][over_cap] indexed by (step - main_levels, slot).  A record that fits neither tier
    // raises *overflow; the host then grows the tier and traces the frame again (fs_capi.cpp).
    float2* over_np; uint32_t* over_mat; float4* over_pos; float4* over_nrm;
    unsigned* overflow;
    uint32_t over_cap;
    int32_t main_levels, over_levels;
    // Staged walks (pipelined depth = 0 frames): a walk that reaches the last step of its stage leaves a continuation
    // record by slot — cont_a = (position, probability of the current node), cont_b = (normal, material | kCont* flags) —
    // and the next stage (one launch later) resumes from it.  Null for walks that run in one piece.
    float4* cont_a; float4* cont_b;
    // FS_FLAG_DOUBLE_POSITIONS: the last node's position in double [total][3] by slot (end_pos keeps the float rounding)
    double* end_posd;
};
constexpr uint32_t kContHasNormal = 1u << 16, kContArrived = 1u << 17, kContAlive = 1u << 18;   // cont_b.w above the 16-bit material

// steps [begin, end) of a walk; slots_cap = the slots this launch has lanes for (a stage that starts at step begin > 0
// only covers the walks longer than that — the first slots of the length-sorted schedule)
struct WalkStage {
    int32_t begin = 0, end = 1 << 30;
    uint32_t slots_cap = 0xFFFFFFFFu;
};
// The long-walk lane of a waited-for staged frame (fs_capi_frame.cpp): the longest walks — those of
// len steps or more, at most cap of them: the FIRST slots of the length-sorted schedule — walk on cooperative waves of
// their own from step 0 on, with their own stage bounds, beside the launch's other walks.  len = 0: no such lane.
struct WalkLane {
    int32_t len = 0;
    uint32_t cap = 0;
    int32_t begin = 0, end = 1 << 30;   // the lane's stage in this launch
    int32_t mode = 0;                   // kLaneBoth / kLaneOnly / kLaneSkip: which of the two classes of slots this part walks
};
constexpr int32_t kLaneBoth = 0, kLaneOnly = 1, kLaneSkip = 2;
constexpr int32_t kLaneSplit = 3;   // (to launch_walk: ONE launch whose first workgroups are the lane's cooperative waves — kLaneOnly — and whose others walk the rest — kLaneSkip)

// host side of DeviceScene.deep: owned by the context, grown by the launchers (attach_deep) when a grid has more lanes
// than the store has columns.  A replaced buffer stays allocated until the scene is freed: launches already in the
// stream still point at it.
struct DeepStore {
    int32_t* buf = nullptr;
    size_t lanes = 0;
    int rows = 0;                       // 0: the committed tree cannot overflow its LDS rows, no store
    std::vector<int32_t*> retired;
    bool failed = false;                // an allocation failed: the launch that needed it was skipped (sticky; fs_synchronize reports it)
};
constexpr int kStackRowsCap = 21;       // LDS rows for pending entries when the tree's worst case needs more (+ 1 row of deep counts)
constexpr int kDeepChunk = 8;           // entries moved per trip to / from the deep store
constexpr int kMaxReconParts = 256;     // reconstruct parts of a fused launch = items of one table slot (fs_context::kReconTabItems)

// ---- host BVH builder ------------------------------------------------------------------------------
struct HostBVH {
    std::vector<NodeQ4> nodes;
    std::vector<Tri64> tris;   // leaf order
    int max_depth = 0;         // of the binary tree before the 4-wide collapse
    int stack_need = 0;        // worst-case pending traversal-stack entries (<= kStackDepth by construction)
    // refit support (fs_refit.hip): input triangle -> leaf-order position; node range [level_begin[l],
    // level_begin[l+1]) of every tree level (breadth-first layout); box padding used by the build
    std::vector<uint32_t> leaf_pos;
    std::vector<int32_t> level_begin;
    float pad = 0.01f;
};
// xyz [T][3][3], mat [T]; binned SAH BVH2 collapsed to a quantised 4-wide tree, <= 2 triangles per leaf.
// cancel (optional): polled by the builder; once set it stops splitting and leaves `out` empty (background builds of
// fs_scene_commit_progressive that a newer registration made useless)
void build_bvh(const float* xyz, const uint16_t* mat, const uint32_t* object_id, int32_t T, HostBVH& out,
               const std::atomic<bool>* cancel = nullptr);

// ---- kernel launchers (fs_kernels.hip) -----------------------------------------------------------------
struct WalkLaunch {
    int variant;         // 2 = wave work sharing (the only one in a default build); 0 = one subpath per lane (FS_EXPERIMENTS)
    int num_cus;         // compute units of the device
    unsigned* queue_head;  // frame scratch: [0] unused, then plan counts + cursors; zero at launch
    uint32_t* perm;      // [depth + 1][total] subpath indices bucketed by planned (RNG-determined) length: the plan pass's schedule
    int rays_per_wave = 64;   // < 64: sparse waves for small frames (variant 2): a wave owns this many subpaths, the other lanes help
    int coop = 1;             // 1: waves of 1, 2 or 4 subpaths search every ray with ALL the lanes of its group (walk_kernel_coop) instead of
                              //    lane-private descents that hand subtrees to idle lanes; 0: the sparse kernel for every rays_per_wave < 64
};
// subpaths per wave the cooperative walk exists for (groups of 64, 32, 16 lanes)
inline bool coop_rays_per_wave(int r) { return r == 1 || r == 2 || r == 4; }
constexpr int kScratchWords = 1 + 2 * (FS_MAX_DEPTH + 1);
// frame scratch allocation: kScratchWords rearmed every frame, then (8-byte aligned) kNumCounters u64 work
// counters that accumulate until fs_reset_stats: walk segments, connections tested, deposits
constexpr int kCounterWord = (kScratchWords + 1) & ~1;
constexpr int kNumCounters = 12;  // walk segments (observed), connections tested, deposits | level 3: walk node / triangle records, any-hit node / triangle records |
                                  // planned segments | level 3: node-record request instructions of the walk, their active lanes, the distinct 64-B records among those | spare
constexpr int kScratchAllocWords = kCounterWord + 2 * kNumCounters;
// The three passes of a frame as the host hands them around (host only: every launcher unpacks its struct to the arguments of
// its kernel).  A pass launched alone and the same pass as a part of the fused launch are described by the same struct.
// The plan pass: the length-bucketed schedule + FlushEnergyBuffer.  wl.queue_head = the frame's scratch set, wl.perm = the
// schedule the pass writes (plan_shape says whether it does: the counts alone otherwise).  The flush: `zero`, or for a batched
// frame the device table zero_tab of zero_count such buffers, of zero_words words each — 0 when there is nothing to flush.
struct PlanPass {
    KParams kp; WalkLaunch wl;
    float* zero = nullptr; float* const* zero_tab = nullptr; int zero_count = 0, zero_words = 0;
};
// The connect pass.  fixed != nullptr: deterministic mode, deposits go to the [B][bins] u64 fixed-point histogram instead;
// scratch = the frame's scratch set (re-armed by the pass); energy_tab / fixed_tab: per-source buffers of a batched frame (device
// arrays of kp.num_local / kp.pairs_per_source pointers), null for one source (`energy` / `fixed` are used).
struct ConnectPass {
    KParams kp; SubpathState st;
    float* energy = nullptr; unsigned long long* fixed = nullptr; unsigned* scratch = nullptr; int pairs_per_wave = 64;
    float* const* energy_tab = nullptr; unsigned long long* const* fixed_tab = nullptr;
};
struct WalkPart {   // a frame's walks from step stage.begin up to step stage.end
    KParams kp; SubpathState st; WalkLaunch wl;   // wl.queue_head = the frame's scratch set, wl.rays_per_wave
    const uint32_t* perm = nullptr;               // its schedule (nullptr: none)
    WalkStage stage;
};
// returns the bucket array to walk through, or nullptr — and zeroes nothing — when there is no roulette to plan for (the caller
// then clears the energy buffer itself)
const uint32_t* launch_plan(const PlanPass& p, hipStream_t s);
// Pipelined frames: ONE launch with several parts — walks (or walk stages) of frames planned before, the connect pass
// of an older one (walked before), the plan pass of the newest.  false = no fused form for this shape (lobes, counting
// instantiations, experiment walk variants, nothing to do): the caller launches the kernels one after the other.
constexpr int kMaxWalkParts = 8;   // walk parts of one fused launch = stages of a staged walk in flight
constexpr int kSlotMaskOffsetWords = 16;  // the mask table starts this many 32-bit words behind the ticket cell (one device allocation)
constexpr int kMaxMaskSources = 1024;     // sources (by handle) whose ring slots have zero-block masks; later ones always write every block
struct PublishWord { unsigned* tickets = nullptr; unsigned long long* host_word = nullptr; unsigned long long id = 0; };
struct FrameParts {
    int num_walk = 0;           // walk parts, in grid order
    WalkPart walk[kMaxWalkParts];
    bool has_connect = false;
    ConnectPass connect;
    bool has_plan = false;
    PlanPass plan;
    // reconstruct parts: ReconstructImpulseResponse of the frames the PREVIOUS launch connected (single GPU; a sharded
    // frame is reduced on the tail stream first and reconstructed there)
    // a table of ReconItem in pinned host memory (fs_context::h_recon_tab: the parts read their item across the bus, as the batch
    // kernel does — the launch's 4 KB of arguments hold no per-item data, so a launch carries as many reconstructs as are owed:
    // cfg5's eight sources per frame no longer fall back to kernels of their own on the tail stream).  ir_bands / ir_mono =
    // nullptr for a frame whose IR is superseded within the launch; host = the pinned ring slot (the publish).
    int num_recon = 0;
    const struct ReconItem* recon_tab = nullptr;
    int recon_B = 0, recon_nb = 0, recon_samples = 0;
    const float* recon_carrier = nullptr;   // the context's carriers if some item is spectral: the fused kernel's spectral instantiation
    // the publish of those host slots (fs_dev_recon.hpp: publish_arrive): the ticket cell, the pinned host word, this launch's id (tickets == nullptr: by an event)
    PublishWord pub;
};
bool launch_frame(int B, const DeviceScene& sc, const FrameParts& f, hipStream_t s);
// does this frame have a plan pass (roulette on, not empty)?  blocks / sort: its grid and whether it writes the schedule
bool plan_shape(const KParams& kp, const WalkLaunch& wl, uint32_t* blocks, bool* sort);
void launch_walk(const DeviceScene& sc, const WalkPart& w, hipStream_t s, const WalkLane& lane = WalkLane());
// can a staged frame whose first stage launches like `first` and whose later ones like `late` have a long-walk lane
// (WalkLane)?  (sparse first stage, cooperative later stages, a cooperative view of the tree for one walk per wave)
bool walk_lane_possible(const DeviceScene& sc, const KParams& kp, const WalkLaunch& first, const WalkLaunch& late, const uint32_t* perm);
// lanes a walk stage needs: all subpaths for a stage that starts at step 0, else the expected number of walks longer than
// stage.begin under the roulette (x1.3 + 1024: the count is binomial, the margin is hundreds of standard deviations)
uint32_t walk_stage_slots(const KParams& kp, int begin);
// dir != nullptr: a directional source (the directional entries, connect_dir_kernel / connect_all_dir_kernel)
void launch_connect(int B, const DeviceScene& sc, const ConnectPass& c, hipStream_t s, const DirArgs* dir = nullptr);
// row f3: every forward prefix x every backward prefix of each pair (one wave per pair), uniform MIS weights — of ONE source:
// the pass's pairs per wave and tables are not read
void launch_connect_all(int B, const DeviceScene& sc, const ConnectPass& c, hipStream_t s, const DirArgs* dir = nullptr);
void launch_fixed_to_energy(const unsigned long long* fixed, float* energy, int words, hipStream_t s);
// carrier != nullptr (FS_FLAG_SPECTRAL_IR): row B is the spectral channel from the [B][carrier_stride] carrier set (fs_dev_recon.hpp:
// reconstruct_spectral_row); the band rows are the same either way
void launch_reconstruct(const float* energy, int B, int num_bins, int sample_rate, int num_samples, int spb,
                        float* ir_bands, float* ir_mono, hipStream_t s, const float* carrier = nullptr);
// ReconstructImpulseResponse of MANY sources as one launch (fs_reconstruct_impulse_response_batch_async): a table of items in
// pinned host memory (read by the kernel as it stands); host != nullptr: the channel view is also written straight into
// that pinned host buffer (the publish: 16-byte stores, a block's 4 096 samples staged in LDS) — no copy command per source.
// mask (optional): the device word that says which 4 096-sample blocks of the host slot may hold non-zero samples (bit b = block b):
// a block whose samples are all exactly zero is not written across the bus again when the slot's block is known to be zero.
// spectral != 0 (FS_FLAG_SPECTRAL_IR): the item's channel row is the spectral IR from the launch's carrier set; 0 = the band mean
struct ReconItem { const float* energy; float* ir_bands; float* ir_mono; float* host; uint32_t* mask; int32_t spb; int32_t spectral; };
// pub.tickets != nullptr: the launch announces its own completion in the context's pinned host word (publish_arrive)
// carrier: the context's carrier set (FS_FLAG_SPECTRAL_IR) for the items marked spectral (nullptr: none is)
// room != nullptr (FS_FLAG_ROOM_PARAMETERS): room[i] = item i's [B] fs_room_parameters records in its pinned host ring slot, a table
// parallel to `table` in pinned host memory; the launch gets count * B more workgroups that compute and write them before it publishes
void launch_reconstruct_batch(const ReconItem* table, int count, int B, int num_bins, int num_samples, hipStream_t s, const PublishWord& pub = PublishWord(),
                              const float* carrier = nullptr, float* const* room = nullptr, float bin_duration = 0.0f);
// FS_FLAG_ROOM_PARAMETERS on its own (the tail stream's reconstruct_now): the [B] records of the [B][num_bins] histogram into host_out
void launch_room_parameters(const float* energy, int B, int num_bins, float bin_duration, float* host_out, hipStream_t s);
// one record: the fields of fs_room_parameters; LDS of a workgroup that computes one (fs_dev_recon.hpp: room_parameters_band):
// the band row [num_bins] floats | kRoomRows rows of kBlock doubles + one — never more than recon_lds_bytes(num_bins)
constexpr int kRoomFields = 9;
static_assert(sizeof(fs_room_parameters) == sizeof(float) * kRoomFields, "fs_room_parameters: nine floats");
constexpr int kRoomRows = 14;
constexpr size_t room_lds_bytes(int num_bins) {
    return sizeof(float) * (((size_t)num_bins + 1) & ~(size_t)1) + sizeof(double) * ((size_t)kRoomRows * kBlock + 1);
}
static_assert(room_lds_bytes(1) <= recon_lds_bytes(1) && room_lds_bytes(2) <= recon_lds_bytes(2),
              "the room-parameter workgroups of a batch run with the reconstruct's LDS");
void launch_trace_rays(const DeviceScene& sc, const float* o, const float* d, const float* tmax, int N, int any_hit,
                       int32_t* hit, float* t, int32_t* tri, float* normal, hipStream_t s);
// rays_per_wave < 64: sparse waves whose other lanes help with every closest-hit query; 64 = one ray per lane
void launch_update_sound(const DeviceScene& sc, const SoundKParams& sp, SoundAccum* acc, int rays_per_wave, hipStream_t s);
// The path queries' kernel arguments.  What the queries share on the device — the chain, the scan, pair and confirm scaffolds, the
// launches — is described in fs_dev_paths.hpp, each query's own kernels in its .hip file; here is what the host fills in.
// The common head (fs_dev_paths.hpp reads nothing else of a first-order query): src = the rows' sources, xyz + the source's actor id as
// bits; lis, lis_object = the listener and its actor; count rows.
struct PathKHead {
    const float4* src;
    float lis[3];
    uint32_t lis_object;
    int32_t count, num_bands;
    float step, pullback, dist_divisor, sound_speed;
};
// fs_direct.hip (fs_update_direct_paths): a wave per source row, lane k = sample k.  h.src lies in pinned host memory (read in
// place); offsets = the [samples][3] table of the call's n (device); out = the device staging the rows are written to.  samples is
// already 1 for a point source.
struct DirectKParams {
    PathKHead h;
    const float* offsets;
    fs_direct_path* out;
    int32_t samples, max_surfaces;
    float radius;
};
void launch_direct_paths(const DeviceScene& sc, const DirectKParams& dp, hipStream_t s);
// fs_reflect.hip (fs_update_reflection_paths): scan and confirm.  h.src on the device; counters [count] zeroed ahead of the scan; cand
// [count][max_candidates] leaf positions; rows [count] and paths [count][max_paths] = the device staging the copy back reads.
struct ReflectKParams {
    PathKHead h;
    uint32_t* counters;
    uint32_t* cand;
    fs_reflection_row* rows;
    fs_reflection_path* paths;
    int32_t max_paths, max_candidates;
    float margin, offset;
};
void launch_reflection_paths(const DeviceScene& sc, const ReflectKParams& rp, hipStream_t s);
// fs_diffract.hip (fs_update_diffraction_paths): scan and confirm; a candidate is leaf position * 4 + edge.  The arrays as
// ReflectKParams; conf [count][max_candidates] = the confirmed records, written and read by the row's wave only.
struct DiffractRecord {
    uint32_t length_bits, key;   // key = input index * 4 + edge
    float apex[3], direction[3];
    float detour, cos_bend;
    uint32_t material, kept;
};
static_assert(sizeof(DiffractRecord) == 48, "DiffractRecord: twelve words");
struct DiffractKParams {
    PathKHead h;
    uint32_t* counters;
    uint32_t* cand;
    DiffractRecord* conf;
    fs_diffraction_row* rows;
    fs_diffraction_path* paths;
    int32_t max_paths, max_candidates;
    float margin, max_detour, offset, merge;
    float k[FS_MAX_BANDS];   // k_b = 40 f_b / (sound_speed dist_divisor)
};
void launch_diffraction_paths(const DeviceScene& sc, const DiffractKParams& dp, hipStream_t s);
// What the pair scaffold reads of a second-order query: near_counters [count] and counters [count], zeroed ahead of the scan; near
// [count][max_near] = the rows' near lists (the scan's codes); cand [count][max_candidates] = the surviving pairs, two near-list slots
// packed 15 + 15 bits.
struct NearPairLists {
    uint32_t* near_counters;
    uint32_t* counters;
    uint32_t* near;
    uint32_t* cand;
    int32_t max_near, max_candidates;
};
// fs_reflect2.hip (fs_update_reflection2_paths): near scan, pair tests and confirm; a near code is a leaf position.  h.src, rows, paths
// as ReflectKParams; conf as DiffractKParams.
struct Reflect2Record {
    uint32_t length_bits, a, b;   // a, b = input indices
    float pa[3], pb[3], direction[3];
    uint32_t material[2];
};
static_assert(sizeof(Reflect2Record) == 56, "Reflect2Record: fourteen words");
struct Reflect2KParams {
    PathKHead h;
    Reflect2Record* conf;
    fs_reflection2_row* rows;
    fs_reflection2_path* paths;
    int32_t max_paths;
    NearPairLists l;
    float max_length, margin, offset;
};
void launch_reflection2_paths(const DeviceScene& sc, const Reflect2KParams& rp, hipStream_t s);
// fs_diffract2.hip (fs_update_diffraction2_paths): near scan, pair tests (q, p; q high) and confirm; a near code is leaf position * 4
// + edge.  The arrays as Reflect2KParams.
struct Diffract2Record {
    uint32_t length_bits, kp, kq;   // kp, kq = input index * 4 + edge of the listener's and the source's edge record
    float apex[2][3], direction[3];
    float detour, gap, cos_bend[2];
    uint32_t material[2];
    uint32_t kept;
};
static_assert(sizeof(Diffract2Record) == 76, "Diffract2Record: nineteen words");
struct Diffract2KParams {
    PathKHead h;
    Diffract2Record* conf;
    fs_diffraction2_row* rows;
    fs_diffraction2_path* paths;
    int32_t max_paths;
    NearPairLists l;
    float margin, max_detour, min_parallel, offset, merge;
    float k[FS_MAX_BANDS];      // k_b = 40 f_b / (sound_speed dist_divisor)
    float lam5[FS_MAX_BANDS];   // lam5_b = 5 sound_speed dist_divisor / f_b
};
void launch_diffraction2_paths(const DeviceScene& sc, const Diffract2KParams& dp, hipStream_t s);
// fs_mixed.hip (fs_update_mixed_paths): near scan, filter (edge record held, face streamed, both ends) and confirm.  A near code is
// leaf position * 4 + edge for an edge record and leaf position * 4 + 3 for a face; a candidate carries its end above the two slots.
// The arrays as Reflect2KParams.
struct MixedRecord {
    uint32_t length_bits, end, m, kr;   // m = the reflector's input index, kr = input index * 4 + edge of the edge record
    float apex[3], point[3], direction[3];
    float detour, bend_detour, cos_bend;
    uint32_t material[2];
    uint32_t kept;
};
static_assert(sizeof(MixedRecord) == 76, "MixedRecord: nineteen words");
struct MixedKParams {
    PathKHead h;
    MixedRecord* conf;
    fs_mixed_row* rows;
    fs_mixed_path* paths;
    int32_t max_paths;
    NearPairLists l;
    float max_length, max_detour, margin, offset, merge;
    float k[FS_MAX_BANDS];      // k_b = 40 f_b / (sound_speed dist_divisor)
};
void launch_mixed_paths(const DeviceScene& sc, const MixedKParams& mp, hipStream_t s);
// fs_pathing.hip (fs_pathing_bake, fs_update_pathing_paths).  The probe set on the device: probes [n] as xyz0; upper and graph, two
// bit matrices [n][stride] with stride = 2 ceil(n / 64) words (a row is whole 64-bit ballots) — the bake's first kernel writes the
// pieces of `upper` on and above the diagonal's block, the mirror kernel reads them and writes every word of `graph`; dL [n], d [n]
// and pred [n] = the listener's attach distances, distances and predecessors of the update in flight.
constexpr int kPathingStrideWords = 2 * ((FS_MAX_PATHING_PROBES + 63) / 64);
struct PathingSet {
    const float4* probes;
    uint32_t* upper;
    uint32_t* graph;
    float* dL;
    float* d;
    uint32_t* pred;
    int32_t n, stride;
};
// the bake: h.step is the bake's, both actor ids FS_NO_OBJECT
struct PathingBakeKParams {
    PathKHead h;
    PathingSet g;
    float max_edge;
};
void launch_pathing_bake(const DeviceScene& sc, const PathingBakeKParams& bp, hipStream_t s);
// the update: h as the other queries' (src on the device), out [count] = the device staging the copy back reads
struct PathingKParams {
    PathKHead h;
    PathingSet g;
    fs_pathing_path* out;
    int32_t validate;
    float max_attach, max_length;
    float k[FS_MAX_BANDS];      // k_b = 40 f_b / (sound_speed dist_divisor)
};
void launch_pathing_paths(const DeviceScene& sc, const PathingKParams& pp, hipStream_t s);
constexpr int kReverbRing = 65536;   // per-channel history ring (floats), matches kRevRing in the kernels
// fs_reverb.hip (the reverb callback): one descriptor per row of the call, in list order, read by every kernel of the callback.
struct ReverbItem {
    const float* ir;       // the convolution's IR (h_from while a crossfade runs) ...
    const float* ir_to;    // ... and the IR it fades to (null: one convolution)
    float* ring;           // history rings [2][kReverbRing]
    float* take_from;      // a source that takes a newer IR in this callback (launch_reverb_batch_fade_start):
    float* take_to;        //   h_from := (1 - take_a) h_from + take_a h_to (take_a > 0), then h_to := take_ir
    const float* take_ir;
    unsigned head;         // ring write head before this callback
    int32_t fade_pos, fade_len;
    float take_a;
    int32_t apply;         // 0: the bypass (out row := in row, nothing else)
    int32_t engine;        // FS_REVERB_ENGINE_*: a PARTITIONED row has its descriptor in the ReverbPartItem table; of this one
                           // it fills apply and engine only, and the direct engine's kernels leave the row alone
};
static_assert(sizeof(ReverbItem) == 72, "ReverbItem: six pointers and six words, the host's staging layout");
// fs_reverb_part.hip (FS_REVERB_ENGINE_PARTITIONED): the descriptor of row i of the call is pitems[i]; active == 0 for every row
// that is not a convolved row of this engine.  A source's state is one block of float2 (Source::d_ring), all spectra in the
// transforms' bit-reversed order: the window history ring (left + i right, or the mono downmix), the literal-tail window's spectrum,
// the products and the delay line of window spectra (the accessors below).
struct ReverbPartItem {
    const float2* h;       // partition spectra [K][N] (H_from while a crossfade runs) ...
    const float2* h_to;    // ... and those it fades to (null: one product)
    float2* state;
    float2* take_from;     // a source that takes a newer IR in this callback (launch_reverb_part_take):
    float2* take_to;       //   H_from := (1 - take_a) H_from + take_a H_to (take_a > 0), then H_to := the spectra of take_ir
    const float* take_ir;
    unsigned head;         // history write head before this callback
    int32_t slot;          // delay-line slot this callback's spectrum enters
    int32_t fade_pos, fade_len;
    float take_a;
    int32_t active;
};
static_assert(sizeof(ReverbPartItem) == 72, "ReverbPartItem: six pointers and six words, the host's staging layout");
// The engine's rows come in two kinds.  A STEREO row (plain or with ears) keeps a float2 history and the literal tail's x_now; a
// mono row (the soundfield bus) keeps a float history, N floats = N / 2 float2, and no x_now.  `acc` is the number of
// products a row keeps per IR copy: 1 for a stereo row, P = ceil(C / 2) channel pairs for the bus.  The regions, in float2:
//   hist [N or N / 2] | x_now [N] (stereo) | Y [2][acc][N] the products (H, H_to) | xring [K][N] the delay line;  N = 1 << n.
__host__ __device__ inline float2* part_hist(float2* state) { return state; }   // (mono: read as N floats)
__host__ __device__ inline float2* part_xnow(float2* state, int n) { return state + ((size_t)1 << n); }
__host__ __device__ inline float2* part_y(float2* state, int n, bool stereo) { return state + (stereo ? (size_t)2 << n : (size_t)1 << (n - 1)); }
__host__ __device__ inline float2* part_xring(float2* state, int n, bool stereo, int acc) {
    return stereo ? state + ((size_t)(2 + 2 * acc) << n) : state + ((size_t)1 << (n - 1)) + ((size_t)(2 * acc) << n);
}
constexpr size_t part_state_elems(int n, int K, bool stereo, int acc) {
    return stereo ? (size_t)(2 + 2 * acc + K) << n : ((size_t)1 << (n - 1)) + ((size_t)(2 * acc + K) << n);
}
// the engine's shape in one call: every partitioned row of a call has one frame size and one context, so one N and K
struct ReverbShape {
    const float2* W;                // twiddles of N = 1 << n
    int n, K, frame, ir_size;
};
// the rows of one kind (plain, ears, bus) in a call, by what their product is
struct ReverbLists {
    const int* plain; int n_plain;  // rows with one product ...
    const int* fade; int n_fade;    // ... and with two
};
// fs_reverb_ears_set's carrier set, as the ear kernels read it: c [2][B][ld] fp32 (mid rows, then side rows)
struct ReverbEars {
    const float* c;
    int B, ld;
};
// fs_reverb_soundfield_set's carrier set, as the soundfield kernels read it: c [C][B][ld] fp32, channel c's B rows car_{c,b};
// w[l] = 1.0f / sqrtf((float)(2 l + 1)), the SN3D diffuse-field weight of degree l, rounded on the host
struct ReverbSoundfield {
    const float* c;
    int B, ld, C;
    float w[4];
};
struct ReverbBatch {
    const ReverbItem* items;        // [count]
    const int* plain; int n_plain;  // rows convolved with one IR ...
    const int* fade; int n_fade;    // ... and with two
    int count, frame, ir_size, literal_tail;
    const float* in;                // [count][2 * frame] interleaved
    float* cur;                     // [count][2][frame] scratch
    float* out;                     // [count][2 * frame] interleaved
    float* mix;                     // [2 * frame], or null
    int n_direct;                   // convolved rows of the direct engine + bypassed rows: what the prepare pass serves
    const ReverbPartItem* pitems;   // [count]: the rows of the partitioned engine (null: none in this call)
    ReverbShape part;
    // its plain rows, and the rows of sources with ears (fs_reverb_set_ears): two spectrum sets per IR copy — ReverbPartItem::h,
    // h_to, take_from, take_to each [2][K][N], M_p then S_p; take_ir = the source's B band rows
    ReverbLists part_rows, ear_rows;
};
// take: the rows whose crossfade starts in this callback (n_take >= 1), n = IR samples
void launch_reverb_batch_fade_start(const ReverbItem* items, const int* take, int n_take, int n, hipStream_t s);
// prepare (+ push, where the ring allows), the convolutions of the two lists (each launched only when it has rows), the push
// (where it could not ride in front), the partitioned engine's rows (launch_reverb_part, when b.pitems), the mix (when b.mix)
void launch_reverb_batch(const ReverbBatch& b, hipStream_t s);
// the mix of the audio callbacks (the reverb's, the direct sound's, the voice banks'): mix [row] = the fp32 sum of out [count][row]
// over the rows, in list order; row = a row's length in floats (2 * frame, or C * frame of the ambisonic bus)
void launch_callback_mix(const float* out, int count, int row, float* mix, hipStream_t s);
// take: the partitioned rows that take a newer IR in this callback (n_take >= 1), one launcher per row kind
void launch_reverb_part_take(const ReverbPartItem* items, const int* take, int n_take, const ReverbShape& p, hipStream_t s);
void launch_reverb_ears_take(const ReverbPartItem* items, const int* take, int n_take, const ReverbShape& p, const ReverbEars& e, hipStream_t s);
void launch_reverb_soundfield_take(const ReverbPartItem* items, const int* take, int n_take, const ReverbShape& p, const ReverbSoundfield& e,
                                   hipStream_t s);
// fs_reverb_copy_ear_impulse_responses: left = m + s, right = m - s of the B band rows `bands` ([B][n]), with the take's expression
void launch_reverb_ears_ir(const float* bands, const ReverbEars& e, int n, float* left, float* right, hipStream_t s);
// fs_reverb_copy_soundfield_impulse_responses: out [C][n] = h_c of the B band rows `bands` ([B][n]), with the take's expression
void launch_reverb_soundfield_ir(const float* bands, const ReverbSoundfield& e, int n, float* out, hipStream_t s);
// the stereo rows: the window transforms, the products of the four lists (each launched only when it has rows), the inverse and epilogue
void launch_reverb_part(const ReverbPartItem* items, const ReverbShape& p, const ReverbLists& rows, const ReverbLists& ears, int count,
                        int literal_tail, const float* in, float* out, hipStream_t s);
// the soundfield rows (fs_reverb_soundfield_process_batch: every row of the call is one, items [count] with h, h_to, take_from, take_to
// each [P][K][N]): the mono window transforms, the products of the two lists, the P inverses per row and the mix (when mix).
// in [count][2 * frame] interleaved stereo; out [count][frame * C], element s * C + c; mix [frame * C], or null
void launch_reverb_soundfield(const ReverbPartItem* items, const ReverbShape& p, const ReverbLists& rows, const ReverbSoundfield& e, int count,
                              const float* in, float* out, float* mix, hipStream_t s);
// fs_direct_render.hip (the direct-sound callback).  A source's state is one device block (Source::dr.d): this header, then at
// kDirectRenderHeader bytes the two history rings [2][ring] (ring a power of two); zeroed = not primed, nothing heard yet.
struct DirectRenderState {
    unsigned n0;           // absolute index of the next block's first sample (wraps; the ring index is n & mask)
    float d0;              // the delay the last output sample used, in samples
    int32_t primed;        // 0: the next callback takes its target without a ramp
    int32_t pad;
    float g0[FS_MAX_BANDS];   // the gains the last output sample used
};
constexpr size_t kDirectRenderHeader = 64;
static_assert(sizeof(DirectRenderState) == 48 && sizeof(DirectRenderState) <= kDirectRenderHeader, "DirectRenderState: twelve words in front of the rings");
// one descriptor per row of the call, in list order: the host's staging layout
struct DirectRenderItem {
    DirectRenderState* state;
    float* ring;           // [2][mask + 1]
    const float* table;    // the band kernels [bands][taps] the source was initialised with
    unsigned mask;
    float d1;              // the row's target: delay in samples, gains
    float g1[FS_MAX_BANDS];
};
static_assert(sizeof(DirectRenderItem) == 64, "DirectRenderItem: three pointers and ten words, the host's staging layout");
// what the plan pass fixes for a row: the state before this callback (its target where the source was not primed) and the
// slew-limited change of the delay over the block
struct DirectRenderPlan {
    unsigned n0;
    float d0, e;
    int32_t pad;
    float g0[FS_MAX_BANDS];
};
struct DirectRenderBatch {
    const DirectRenderItem* items;  // [count]
    DirectRenderPlan* plans;        // [count] scratch
    int count, frame, taps, bands;
    const float* in;                // [count][2 * frame] interleaved
    float* out;                     // [count][2 * frame] interleaved
    float* mix;                     // [2 * frame], or null
};
// the plan pass, the render pass (which also appends the blocks to the rings), the mix (when b.mix)
void launch_direct_render(const DirectRenderBatch& b, hipStream_t s);
// The voice bank (fs_dev_render.hpp: its two passes; fs_capi_voice_bank.hpp: its host side), which the early-reflection and the
// binaural callback are built on: per source a table of kVoiceSlots slots, each a voice — a delay, band gains and what the renderer's
// voices carry beyond them — held from callback to callback.  A source's state is one device block (Source::rr.r.d / br.r.d): a
// VoiceBankState of the renderer's slot record, then at kVoiceBankHeader bytes the two history rings [2][ring], shared by the
// source's slots; zeroed = every slot free, nothing heard.
constexpr int kVoiceSlots = FS_MAX_REFLECTION_VOICES;
template <typename Slot>
struct VoiceBankState {
    unsigned n0;           // absolute index of the next block's first sample (wraps; the ring index is n & mask)
    int32_t pad[15];
    Slot slot[kVoiceSlots];
};
constexpr size_t kVoiceBankHeader = 2304;
// what the host's matching decided for a slot in this callback (VoiceBankItem::op): idle, ending, or continuing / starting
// with entry e of the row as kVoiceContinue + e / kVoiceStart + e
constexpr int kVoiceIdle = -1, kVoiceEnd = -2, kVoiceContinue = 0, kVoiceStart = kVoiceSlots;
// one descriptor per row of the call, in list order: the host's staging layout
template <typename Slot>
struct VoiceBankItem {
    VoiceBankState<Slot>* state;
    float* ring;           // [2][mask + 1]
    const float* table;    // the band kernels [bands][taps] the source was initialised with
    unsigned mask;
    int32_t slots;         // V
    int8_t op[kVoiceSlots];
};
// fs_reflect_render.hip (the early-reflection callback): a voice carries a pair of channel gains
struct ReflectRenderSlot {
    int32_t held;          // the device's record of the slot table; the matching itself runs on the host's copy (VoiceBank::held / key)
    uint32_t key;
    float d0;              // the delay the slot's last output sample used, in samples
    float g0[FS_MAX_BANDS];   // ... its band gains
    float w0[2];           // ... its channel gains
    int32_t pad[3];
};
static_assert(sizeof(ReflectRenderSlot) == 64, "ReflectRenderSlot: sixteen words");
using ReflectRenderState = VoiceBankState<ReflectRenderSlot>;
static_assert(sizeof(ReflectRenderState) == 2112 && sizeof(ReflectRenderState) <= kVoiceBankHeader && kVoiceBankHeader % 256 == 0,
              "VoiceBankState: the counter's line and the slots in front of the rings");
struct ReflectRenderItem : VoiceBankItem<ReflectRenderSlot> {};
static_assert(sizeof(ReflectRenderItem) == 64, "ReflectRenderItem: three pointers, two words and a byte per slot, the host's staging layout");
// what the plan pass fixes for a sounding slot: where this callback ramps from, the slew-limited change of the delay, the gains
// it ramps between and the channel gains' start and change
struct ReflectRenderPlan {
    float d0, e;
    float g0[FS_MAX_BANDS], g1[FS_MAX_BANDS];
    float w0[2], dw[2];
    int32_t pad[2];
};
static_assert(sizeof(ReflectRenderPlan) == 96, "ReflectRenderPlan: twenty-four words");
struct ReflectRenderBatch {
    const ReflectRenderItem* items;     // [count]
    const fs_reflection_voice* voices;  // [count][stride]
    ReflectRenderPlan* plans;           // [count][kVoiceSlots] scratch
    unsigned* n0;                       // [count] scratch: every row's counter before this callback
    int count, stride, frame, taps, bands;
    float fs;                           // the sample rate: an entry's d1 = delay * fs
    const float* in;                    // [count][2 * frame] interleaved
    float* out;                         // [count][2 * frame] interleaved
    float* mix;                         // [2 * frame], or null
};
// the plan pass, the render pass (which also appends the blocks to the rings), the mix (when b.mix)
void launch_reflect_render(const ReflectRenderBatch& b, hipStream_t s);
// fs_binaural_render.hip (the binaural-voice callback): a voice carries one gain and the index of its HRIR
struct BinauralRenderSlot {
    int32_t held;          // as ReflectRenderSlot's
    uint32_t key;
    float d0;              // the delay the slot's last output sample used, in samples
    float g0[FS_MAX_BANDS];   // ... its band gains
    float w0;              // ... its gain
    int32_t q0;            // ... its HRIR index
    int32_t pad[3];
};
static_assert(sizeof(BinauralRenderSlot) == 64, "BinauralRenderSlot: sixteen words");
using BinauralRenderState = VoiceBankState<BinauralRenderSlot>;
static_assert(sizeof(BinauralRenderState) == 2112, "VoiceBankState: one layout, whatever the sixteen words of a slot hold");
// first = the index in the call's folded tables of the row's lowest sounding slot, the others follow in ascending slot number
struct BinauralRenderItem : VoiceBankItem<BinauralRenderSlot> {
    int32_t first;
    int32_t pad;
};
static_assert(sizeof(VoiceBankItem<BinauralRenderSlot>) == 64 && sizeof(BinauralRenderItem) == 72,
              "BinauralRenderItem: three pointers, two words, a byte per slot, two words: the host's staging layout");
// what the plan pass fixes for a sounding slot: where this callback ramps from, the slew-limited change of the delay, the gains
// it ramps between, the gain's start and change, the HRIR indices it fades between, its index in the folded tables
struct BinauralRenderPlan {
    float d0, e;
    float g0[FS_MAX_BANDS], g1[FS_MAX_BANDS];
    float w0, dw;
    int32_t q0, q1;
    int32_t index;
    int32_t pad;
};
static_assert(sizeof(BinauralRenderPlan) == 96, "BinauralRenderPlan: twenty-four words");
// The mesh on the HRIR set in force (fs_hrtf_set_mesh): the header's locate rule, to the bit, for the host (fs_hrtf_mesh_locate)
// and the device (the locate pass) alike — every operation fp32, rounded on its own, in the order written.  Rows r_0, r_1, r_2 of
// triangle j come through `rows(j, i)`: the host reads the caller's [m][3][3], the device the mesh
// block's [m][3] float4 {r_i.x, r_i.y, r_i.z, the bits of corner v_i}: a lane's triangle is three 16-byte requests, and a wave's 64
// triangles are 3 KiB in one piece.
struct HrtfMeshBest { float mu; int j; };
struct HrtfMeshRow { float x, y, z; };
struct HrtfMeshRowsHost {
    const float* rows;   // [m][3][3]
    __host__ __device__ HrtfMeshRow operator()(int j, int i) const {
        const float* r = rows + ((size_t)j * 3 + (size_t)i) * 3;
        return {r[0], r[1], r[2]};
    }
};
struct HrtfMeshRowsDevice {
    const float4* mesh;  // [m][3]
    __host__ __device__ HrtfMeshRow operator()(int j, int i) const {
        const float4 q = mesh[(size_t)j * 3 + (size_t)i];
        return {q.x, q.y, q.z};
    }
};
__host__ __device__ inline float hrtf_mesh_g(const HrtfMeshRow& r, const float* d) { return (d[0] * r.x + d[1] * r.y) + d[2] * r.z; }
// does a replace b as the best triangle: the larger mu, among equals the lower index
__host__ __device__ inline bool hrtf_mesh_better(const HrtfMeshBest& a, const HrtfMeshBest& b) {
    return a.mu > b.mu || (a.mu == b.mu && a.j < b.j);
}
// steps 1 and 2 over triangles first, first + step, ... < m, from best = (-infinity, 0): the host walks all of them (0, 1), lane l
// of a wave every 64th (l, 64); hrtf_mesh_better merges the lanes' answers into the host's — a mu that is not a number is never taken
template <typename Rows>
__host__ __device__ inline HrtfMeshBest hrtf_mesh_scan(const Rows& rows, int m, const float* d, int first, int step) {
    HrtfMeshBest best = {-INFINITY, 0};
#pragma unroll 4   // (the device: four triangles' rows in flight per lane; the comparisons stay in ascending j)
    for (int j = first; j < m; j += step) {
        const float g0 = hrtf_mesh_g(rows(j, 0), d), g1 = hrtf_mesh_g(rows(j, 1), d), g2 = hrtf_mesh_g(rows(j, 2), d);
        float mu = g0;
        if (g1 < mu) mu = g1;
        if (g2 < mu) mu = g2;
        if (mu > best.mu) { best.mu = mu; best.j = j; }   // (ascending j: an equal later one does not replace it)
    }
    return best;
}
// step 3 for triangle t
template <typename Rows>
__host__ __device__ inline void hrtf_mesh_weights(const Rows& rows, int t, const float* d, float* b) {
    const float g0 = hrtf_mesh_g(rows(t, 0), d), g1 = hrtf_mesh_g(rows(t, 1), d), g2 = hrtf_mesh_g(rows(t, 2), d);
    const float c0 = g0 > 0.0f ? g0 : 0.0f, c1 = g1 > 0.0f ? g1 : 0.0f, c2 = g2 > 0.0f ? g2 : 0.0f;
    const float s = (c0 + c1) + c2;
    if (s > 0.0f) { b[0] = c0 / s; b[1] = c1 / s; b[2] = c2 / s; }
    else { b[0] = 1.0f; b[1] = 0.0f; b[2] = 0.0f; }
}
// With a mesh in force a slot's q0, pad[3] hold t0 and the bits of b0[3] (BinauralRenderSlot keeps its layout), and the plan is a
// wider record: BinauralRenderPlan's twenty-four words (q0, q1 unused), then the triangles and weights the callback fades between.
struct BinauralMeshPlan : BinauralRenderPlan {
    int32_t t0, t1;
    float b0[3], b1[3];
};
static_assert(sizeof(BinauralMeshPlan) == 128, "BinauralMeshPlan: thirty-two words");
// Onsets on the set in force (fs_hrtf_set_onsets): the header's delayed HRIR, to the bit, for the host (fs_hrtf_delay) and the
// device (the fold's LDS fill) alike — every operation fp32, rounded on its own, in the order written.  tau = i + f, i = (int)tau;
// tap k of the delayed HRIR is g * x(k - i) + f * x(k - i - 1) with g = 1.0f - f, where `x(j)` gives the aligned HRIR's tap j and
// 0.0f outside 0 .. H-1: the host reads the caller's array, the device the set's — or, with a mesh, blends three as it reads.
struct HrtfDelay { int i; float f, g; };
__host__ __device__ inline HrtfDelay hrtf_delay_of(float tau) {
    const int i = (int)tau;
    const float f = tau - (float)i;
    return {i, f, 1.0f - f};
}
template <typename X>
__host__ __device__ inline float hrtf_delay_tap(const HrtfDelay& d, int k, const X& x) {
    return d.g * x(k - d.i) + d.f * x(k - d.i - 1);
}
struct BinauralRenderBatch {
    const float* onsets;                // the onsets in force: [n_dirs][2] samples; null: none, omax unused and h_eff == h_taps
    float omax;                         // ... the largest of them
    int h_eff;                          // He = h_taps + (int)omax + 1: the taps of a delayed HRIR — of the fold, tc = taps + h_eff - 1
    const float4* mesh;                 // the mesh in force: [n_tris][3] {r_i, corner v_i}; null: nearest mode, and the three below unused
    int n_tris;
    float4* located;                    // [count][kVoiceSlots] scratch: {the bits of t1, b1[3]} of every slot with an entry
    BinauralMeshPlan* mesh_plans;       // [count][kVoiceSlots] scratch: in `plans`' place
    const BinauralRenderItem* items;    // [count]
    const fs_binaural_voice* voices;    // [count][stride]
    const uint16_t* sounding;           // [n_sounding]: row * kVoiceSlots + slot of every sounding slot, rows then slots ascending
    BinauralRenderPlan* plans;          // [count][kVoiceSlots] scratch
    unsigned* n0;                       // [count] scratch: every row's counter before this callback
    float2* folded;                     // [n_sounding][2 ears][tc] scratch: {C0[u], dC[u]}
    const float* dirs;                  // the set in force: [n_dirs][3] ...
    const float* hrir;                  // ... [n_dirs][2][h_taps]
    int n_dirs, h_taps;
    int count, stride, frame, taps, tc, bands, n_sounding;
    float fs;                           // the sample rate: an entry's d1 = delay * fs
    const float* in;                    // [count][2 * frame] interleaved
    float* out;                         // [count][2 * frame] interleaved
    float* mix;                         // [2 * frame], or null
};
// (with b.mesh: the locate pass,) the plan pass, the fold of the HRIRs into the band FIRs, the render pass (which also appends the
// blocks to the rings), the mix (when b.mix)
void launch_binaural_render(const BinauralRenderBatch& b, hipStream_t s);
// fs_ambisonic_render.hip (the ambisonic-voice callback): a voice carries the gains of the C = (order + 1)^2 channels of an
// ambisonic bus, ACN order and SN3D normalisation, up to order 3.  A source's state block is a VoiceBankState of 128-byte slots,
// then at kAmbisonicBankHeader bytes ONE history ring [ring]: a point source is mono, x(n) = 0.5f * (left + right).
constexpr int kAmbisonicChannels = 16;
// The header's encoding, to the bit, for the host (fs_ambisonic_encode) and the device (the plan pass) alike: every operation is
// fp32, rounded on its own, in the order written; division and square root are correctly rounded on both.  y [kAmbisonicChannels]:
// the (order + 1)^2 first are written.  The head frame has y to the right, AmbiX to the left: y is negated.
__host__ __device__ inline void ambisonic_encode(int order, const float* d, float* y_out) {
    const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const float x = d[0] / len, y = -(d[1] / len), z = d[2] / len;
    y_out[0] = 1.0f;
    if (order < 1) return;
    y_out[1] = y;
    y_out[2] = z;
    y_out[3] = x;
    if (order < 2) return;
    const float xx = x * x, yy = y * y, zz = z * z;
    const float K3 = (float)1.7320508075688772, K3h = (float)0.8660254037844386;   // sqrt(3), sqrt(3) / 2
    y_out[4] = K3 * (x * y);
    y_out[5] = K3 * (y * z);
    y_out[6] = 1.5f * zz - 0.5f;
    y_out[7] = K3 * (x * z);
    y_out[8] = K3h * (xx - yy);
    if (order < 3) return;
    const float K58 = (float)0.7905694150420949, K15 = (float)3.872983346207417;   // sqrt(5 / 8), sqrt(15)
    const float K38 = (float)0.6123724356957945, K15h = (float)1.9364916731037085;   // sqrt(3 / 8), sqrt(15) / 2
    y_out[9] = K58 * (y * (3.0f * xx - yy));
    y_out[10] = K15 * ((x * y) * z);
    y_out[11] = K38 * (y * (5.0f * zz - 1.0f));
    y_out[12] = z * (2.5f * zz - 1.5f);
    y_out[13] = K38 * (x * (5.0f * zz - 1.0f));
    y_out[14] = K15h * (z * (xx - yy));
    y_out[15] = K58 * (x * (xx - 3.0f * yy));
}
// what the entry points accept as a direction: finite components and an fp32 squared length, summed as above, in [1e-30, 1e30]
inline bool ambisonic_direction_ok(const float* d) {
    if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) return false;
    const float len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    return std::isfinite(len2) && len2 >= 1e-30f && len2 <= 1e30f;
}
struct AmbisonicRenderSlot {
    int32_t held;          // as ReflectRenderSlot's
    uint32_t key;
    float d0;              // the delay the slot's last output sample used, in samples
    float g0[FS_MAX_BANDS];   // ... its band gains
    float w0[kAmbisonicChannels];   // ... its channel gains (0 beyond C)
    int32_t pad[5];
};
static_assert(sizeof(AmbisonicRenderSlot) == 128, "AmbisonicRenderSlot: thirty-two words");
using AmbisonicRenderState = VoiceBankState<AmbisonicRenderSlot>;
constexpr size_t kAmbisonicBankHeader = 4352;
static_assert(sizeof(AmbisonicRenderState) == 4160 && sizeof(AmbisonicRenderState) <= kAmbisonicBankHeader && kAmbisonicBankHeader % 256 == 0,
              "VoiceBankState: the counter's line and 32 slots of 128 bytes in front of the ring");
struct AmbisonicRenderItem : VoiceBankItem<AmbisonicRenderSlot> {};
static_assert(sizeof(AmbisonicRenderItem) == 64, "AmbisonicRenderItem: ReflectRenderItem's layout (ring: [mask + 1], one ring)");
// what the plan pass fixes for a sounding slot: ReflectRenderPlan's, with sixteen channel gains' start and change
struct AmbisonicRenderPlan {
    float d0, e;
    float g0[FS_MAX_BANDS], g1[FS_MAX_BANDS];
    float w0[kAmbisonicChannels], dw[kAmbisonicChannels];
    int32_t pad[14];
};
static_assert(sizeof(AmbisonicRenderPlan) == 256, "AmbisonicRenderPlan: sixty-four words");
struct AmbisonicRenderBatch {
    const AmbisonicRenderItem* items;   // [count]
    const fs_ambisonic_voice* voices;   // [count][stride]
    AmbisonicRenderPlan* plans;         // [count][kVoiceSlots] scratch
    unsigned* n0;                       // [count] scratch: every row's counter before this callback
    int count, stride, frame, taps, bands, order;
    float fs;                           // the sample rate: an entry's d1 = delay * fs
    const float* in;                    // [count][2 * frame] interleaved stereo
    float* out;                         // [count][frame][C]
    float* mix;                         // [frame][C], or null
};
// the plan pass, the render pass (which also appends the blocks' downmix to the rings), the mix (when b.mix)
void launch_ambisonic_render(const AmbisonicRenderBatch& b, hipStream_t s);
void launch_add_energy(float* energy_row, int num_bins, float delay_s, float e, hipStream_t s);
// dynamic LDS the traversal kernels of a frame need for a tree with `stack_rows` stack rows: the larger of the walk
// kernel (stack + work-sharing area) and the connect kernels (stack + [bands][bins] histogram + work-sharing area)
size_t traversal_lds_bytes(int stack_rows, int bands, int num_bins);
int default_hist_window(int bands);   // LDS histogram bins of the connect part when FS_HIST_WINDOW is not set
// fs_oneshot.hip: the sum of a [bands][bins] buffer over the ranks as one peer-write exchange (fs_comm_enable_oneshot).
// A rank's mailbox: kOneShotHeaderBytes of flags ([2 sets][kOneShotMaxRanks] u32 sequence numbers), then
// [2 sets][world] slots of slot_bytes each.  mail[r] = rank r's mailbox as mapped into this process.
constexpr int kOneShotMaxRanks = 16;
constexpr size_t kOneShotHeaderBytes = 256;
struct OneShotView {
    void* mail[kOneShotMaxRanks];
    int32_t world, rank;
    size_t slot_bytes;
};
// buffer: fp32 [words] (or u64 [words], deterministic mode), summed in place over the ranks; set = seq & 1
void launch_oneshot_reduce(const OneShotView& v, void* buffer, int words, bool u64, int set, uint32_t seq, unsigned* err,
                           hipStream_t s);
// row f4 (fs_refit.hip): moving geometry without a rebuild.  xyz = `count` new triangles [count][3][3] on the
// device, written to the leaf-order records through leaf_pos; then one refit launch per tree level, deepest
// first (node_box = scratch [num_nodes][2] float4 holding each node's fp32 bounds).
// view: the 48-byte node view's copies of the records follow (rec / nrm by record number, rec_of_leaf: leaf order -> record), or all null
struct ViewTris { ViewRec* rec; float4* nrm; const uint32_t* rec_of_leaf; };
void launch_update_triangles(Tri64* tris, Tri48* packed, float4* nrm, const uint32_t* leaf_pos, int first, int count,
                             const float* xyz, const ViewTris& view, hipStream_t s);
// fs_scene_set_object_transforms: every triangle of the n listed objects placed at its matrix applied to its rest position
// (rest [T][9] input order; csr / start: the objects' lists of input indices; prefix [n + 1]: running triangle counts;
// *amax_bits: bit pattern of the largest |coordinate| written, kept up by atomicMax)
void launch_transform_objects(Tri64* tris, Tri48* packed, float4* nrm, const uint32_t* leaf_pos, const float* rest,
                              const uint32_t* csr, const uint32_t* prefix, const uint32_t* start, const float* m, int n,
                              uint32_t total, uint32_t* amax_bits, const ViewTris& view, hipStream_t s);
void launch_pack_triangles(const Tri64* tris, int count, Tri48* packed, float4* nrm, hipStream_t s);
void launch_refit(NodeQ4* nodes, const Tri64* tris, float4* node_box, const int32_t* level_begin, int levels, float pad,
                  hipStream_t s);
void launch_coop_nodes(const NodeQ4* nodes, int n, CoopChild* out, hipStream_t s);   // per-child records of the current 4-wide nodes
// ... folded two levels at a time into 16-wide nodes in the dense order of the even levels (fs_refit.hip)
void launch_coop16(const CoopChild* in, const int32_t* level_begin_dev, const int32_t* dense_dev, int levels, int n16, CoopChild* out, hipStream_t s);
// The 48-byte node view (ViewRec above).  launch_node_view_layout (topology only: behind a commit): block[n] = records of
// node n's child block -> exclusive scan -> rec_of_node / rec_of_leaf.  launch_node_view_fill (every commit and refit): the
// records from nodes / tris48 / nrm as they stand in the stream; *bad is raised if a grid step is no encodable power of two.
// block: [nodes + 1] scratch that holds the scan afterwards (kept across refits).
void launch_node_view_layout(const NodeQ4* nodes, int n, int T, uint32_t* block, uint32_t* rec_of_node, uint32_t* rec_of_leaf, hipStream_t s);
void launch_node_view_fill(const NodeQ4* nodes, int n, const Tri48* tris, const float4* nrm, int T, const uint32_t* block,
                           const uint32_t* rec_of_node, const uint32_t* rec_of_leaf, ViewRec* rec, float4* rec_nrm, uint32_t* bad, hipStream_t s);
// fs_build.hip: the acceleration structure built on the device (Morton codes, radix sort, Karras' binary radix tree,
// breadth-first collapse to 4-wide nodes); launch_refit then derives the quantised boxes.  DeviceBuildInfo is what the
// host reads back: levels < 0 = the tree is deeper than kMaxBuildLevels or ran out of node space (use the host build).
constexpr int kMaxBuildLevels = 96;
struct DeviceBuildInfo {
    int32_t num_nodes, levels, stack_need, reserved;
    int32_t level_begin[kMaxBuildLevels + 1];
};
size_t device_build_scratch_bytes(int T);
bool launch_device_build(const float* xyz, const uint16_t* mat, const uint32_t* object_id, int T, const float lo[3],
                         const float hi[3], NodeQ4* nodes, Tri64* tris, uint32_t* leaf_pos, void* scratch, size_t scratch_bytes,
                         DeviceBuildInfo* info_dev, hipStream_t s);
// row f4 (fs_fft.hip): ApplyMaterialFD.  x [N] and y [3][N] complex work buffers, W [N/2] twiddles,
// resp [3][N/2+1] = absorption | transmission | scattering, out [3][L] = specular | diffuse | transmitted
constexpr int kFftChunkLog = 11;     // FFT stages with spans below 2^11 points run inside LDS
void launch_apply_material_fd(const float* in, int L, int n, float2* x, float2* y, const float2* W, const float* resp,
                              float* out, hipStream_t s);
// FS_FLAG_SPECTRAL_IR (fs_fft.hip): the per-band noise carriers the spectral channel row is built from.  Bin k in [1, K/2) of a
// K = 2^n point spectrum belongs to band b when lo[b] <= k < lo[b + 1] (host-side, from the band edges in double); its phase is
// 2 pi (splitmix64(kCarrierSeed + k) >> 40) 2^-24.  out: [B][ld] fp32, ld = carrier_stride(N) (below)
constexpr uint64_t kCarrierSeed = 0x5EED;
constexpr uint64_t kEarSideSeed = 0x5EED0EA2;   // fs_reverb_ears_set: the side carriers' phases psi_k
constexpr int kCarrierMaxLog = 24;   // K <= 2^24 (the material filter's largest transform)
struct CarrierBands { int32_t lo[FS_MAX_BANDS + 1]; };
// a carrier row's length: N rounded up to 64 samples (a whole number of the reconstruct's chunks: 16-byte loads of a thread's own)
__host__ __device__ constexpr int carrier_stride(int num_samples) { return (num_samples + 63) / 64 * 64; }
void launch_build_carriers(int B, int n, int N, int ld, const CarrierBands& bands, float2* X, float2* y, const float2* W,
                           const float* zeros, float* out, hipStream_t s);
void launch_build_ear_carriers(int B, int n, int N, int ld, const CarrierBands& bands, double fs, double radius_cm, double speed_cm_s,
                               float2* X, float2* y, const float2* W, const float* zeros, float* out, hipStream_t s);
// fs_reverb_soundfield_set: C channels of B rows each, channel c's phases from kCarrierSeed + (c << 32) + k.  X, y: [B][K] work
// buffers, used channel after channel; out: [C][B][ld]
void launch_build_soundfield_carriers(int C, int B, int n, int N, int ld, const CarrierBands& bands, float2* X, float2* y, const float2* W,
                                      const float* zeros, float* out, hipStream_t s);

}  // namespace fs
