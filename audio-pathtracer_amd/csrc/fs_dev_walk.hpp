// fs_dev_walk.hpp — the walk (GeneratePath, AudioRayTracingSubsystem.cpp:279-355): walker, segment records, walk stages,
// the plan pass, and the bodies of the walk kernels on dense and on sparse waves.
#pragma once
#include "fs_dev_trav.hpp"

namespace fs {
namespace {

// ---------------------------------------------------------------------------------------------------
// the walk, shared by both kernel variants
// ---------------------------------------------------------------------------------------------------
struct Walker {          // ARTS.cpp:287-291 state + bookkeeping
    uint32_t g, slot, side, li, pair;   // subpath index, launch slot (where its records go), side, pair of the frame, RNG pair
    int k;
    float px, py, pz, nx, ny, nz;
    double dpx, dpy, dpz;   // FS_FLAG_DOUBLE_POSITIONS: the node position as the reference's FVector holds it (px.. = its float rounding)
    bool has_normal;
    bool arrived;      // the current vertex was reached by a hit (lobes are picked only then)
    uint32_t mat;
    uint32_t lobe;     // lobe picked at the current vertex << kLobeShift (FS_FLAG_MATERIAL_LOBES), else 0
    float prob, prob_new;
    uint32_t ign;      // the actor this walk ignores (EXT instantiations; FS_NO_OBJECT: none)
};

// low seed word of item `sid` of a batched frame (grouped frames carry one seed per item; kp.item_seeds <= 4)
__device__ __forceinline__ uint32_t item_seed_lo(const KParams& kp, uint32_t sid) {
    uint32_t s = kp.seed_lo;
    if (kp.item_seeds > 0) {   // (wave-uniform)
        s = kp.item_seed[0];
        s = sid == 1u ? kp.item_seed[1] : s;
        s = sid == 2u ? kp.item_seed[2] : s;
        s = sid == 3u ? kp.item_seed[3] : s;
    }
    return s;
}

// ---- segment records: [step][slot] in the main tier, (step - main_levels, slot) in the overflow tier ------------
__device__ __forceinline__ bool rec_in_main(const SubpathState& st, int k) { return k < st.main_levels; }
__device__ __forceinline__ size_t rec_main(uint32_t total, int k, uint32_t slot) { return (size_t)k * total + slot; }
__device__ __forceinline__ size_t rec_over(const SubpathState& st, int k, uint32_t slot) {
    return (size_t)(k - st.main_levels) * st.over_cap + slot;
}
// does step k of the walk in `slot` have a place?  (always, for a capped depth)
__device__ __forceinline__ bool rec_fits(const SubpathState& st, int k, uint32_t slot) {
    return k < st.main_levels || (slot < st.over_cap && k - st.main_levels < st.over_levels);
}
__device__ __forceinline__ float2 load_np(const SubpathState& st, uint32_t total, int k, uint32_t slot) {
    return rec_in_main(st, k) ? st.seg_np[rec_main(total, k, slot)] : st.over_np[rec_over(st, k, slot)];
}
__device__ __forceinline__ uint32_t load_mat(const SubpathState& st, uint32_t total, int k, uint32_t slot) {
    return rec_in_main(st, k) ? st.seg_mat[rec_main(total, k, slot)] : st.over_mat[rec_over(st, k, slot)];
}
__device__ __forceinline__ float4 load_pos(const SubpathState& st, uint32_t total, int k, uint32_t slot) {
    return rec_in_main(st, k) ? st.seg_pos[rec_main(total, k, slot)] : st.over_pos[rec_over(st, k, slot)];
}
__device__ __forceinline__ float4 load_nrm(const SubpathState& st, uint32_t total, int k, uint32_t slot) {
    return rec_in_main(st, k) ? st.seg_nrm[rec_main(total, k, slot)] : st.over_nrm[rec_over(st, k, slot)];
}
__device__ __forceinline__ void store_mat(const SubpathState& st, uint32_t total, int k, uint32_t slot, uint32_t v) {
    if (rec_in_main(st, k)) st.seg_mat[rec_main(total, k, slot)] = v;
    else if (rec_fits(st, k, slot)) st.over_mat[rec_over(st, k, slot)] = v;
}
// slot of subpath g
__device__ __forceinline__ uint32_t slot_of(const SubpathState& st, uint32_t g) { return st.slot_of ? st.slot_of[g] : g; }

__device__ __forceinline__ void walker_start(Walker& w, uint32_t g, uint32_t slot, const KParams& kp, const SubpathState& st,
                                             bool own = true) {   // own = false: a helper lane without a subpath
    const uint32_t n = kp.num_local;
    w.g = g;
    w.slot = slot;
    if (own && st.slot_of) st.slot_of[g] = slot;   // the connect kernels find the walk's records through this
    w.side = g >= n ? 1u : 0u;
    w.li = g - w.side * n;
    w.pair = kp.pair_begin + w.li;
    w.px = w.side ? kp.lis[0] : kp.src[0];
    w.py = w.side ? kp.lis[1] : kp.src[1];
    w.pz = w.side ? kp.lis[2] : kp.src[2];
    if (kp.src_table) {   // batched frame (wave-uniform): several sources' pairs end to end, same RNG pairs for each
        const uint32_t sid = w.li / kp.pairs_per_source;
        w.pair = kp.pair_begin + (w.li - sid * kp.pairs_per_source);
        if (!w.side) { w.px = kp.src_table[4 * sid]; w.py = kp.src_table[4 * sid + 1]; w.pz = kp.src_table[4 * sid + 2]; }
    }
    w.ign = w.side ? kp.lis_object : kp.src_object;   // AddIgnoredActor ARTS.cpp:322-327 (used by the EXT instantiations only)
    if (kp.src_table && !w.side) w.ign = __float_as_uint(kp.src_table[4 * (w.li / kp.pairs_per_source) + 3]);
    w.dpx = (double)w.px; w.dpy = (double)w.py; w.dpz = (double)w.pz;
    w.nx = 0.f; w.ny = 0.f; w.nz = 0.f;
    w.has_normal = false;
    w.arrived = false;
    w.lobe = 0u;
    w.mat = kNoMat;
    w.prob = 1.0f; w.prob_new = 1.0f;
    w.k = 0;
}

// top of GeneratePath's loop (ARTS.cpp:294-319): depth cap, roulette, direction.  false = the walk ends.
// `ray` still holds the previous segment's ray on entry: its direction is the arrival direction at this vertex.
// LOBES: 0 / 1 = FS_FLAG_MATERIAL_LOBES known at compile time, -1 = read kp.lobes.
// pre: the Philox words of this bounce, computed ahead by another lane (cooperative walk: the roulette and the sample of a
// bounce depend on (seed, pair, side, bounce) only) — the same words, so the same walk.  pre_cone: words y, z, w are already the
// diffuse sample in the cone's own frame (cone_local) — only for a vertex with a normal, without lobes
template <int LOBES = -1>
__device__ __forceinline__ bool walker_next_ray(Walker& w, const KParams& kp, const DeviceScene& sc,
                                                const SubpathState& st, Ray& ray, const uint4* pre = nullptr, const bool pre_cone = false) {
    const bool lobes_on = LOBES < 0 ? kp.lobes != 0 : LOBES != 0;
    if (w.k >= kp.depth && st.over_levels == 0) return false;             // the depth cap
    const uint32_t bs = ((uint32_t)w.k << 1) | w.side;
    // (grouped frames: the item's own low seed word — recomputed from the pair index here, once per bounce, rather than
    // carried in a register through the traversal: one more live VGPR cost the 128-register frame kernel 3 %)
    const uint32_t seed = kp.item_seeds > 0 ? item_seed_lo(kp, w.li / kp.pairs_per_source) : kp.seed_lo;
    const uint4 r = pre ? *pre : philox(w.pair, bs, 0, seed, kp.seed_hi);
    if (kp.russian_roulette && !(u01(r.x) < kp.rr_prob)) return false;    // ARTS.cpp:300-301, 349-353
    if (w.k >= kp.depth) { *st.overflow = 1u; return false; }             // depth = 0 and the walk outlives both tiers
    float dx, dy, dz;
    if (!w.has_normal) {                                                  // ARTS.cpp:306-310
        sample_sphere(w.pair, bs, r, seed, kp.seed_hi, dx, dy, dz);
        float pdf = 1.0f / (4.0f * kPi);
        w.prob_new = pdf * kp.rr_prob;
    } else {                                                              // ARTS.cpp:311-318
        // FS_FLAG_MATERIAL_LOBES (row f4, build-owned): one lobe per vertex, picked with the Philox word the diffuse
        // walk leaves unused, probabilities = band means of the lobe gains (table built at commit)
        uint32_t lobe = kLobeDiffuse;
        float plobe = 1.0f;
        const bool pick = lobes_on && w.arrived && w.mat != kNoMat && (int32_t)w.mat < sc.num_materials;
        if (pick) {
            const float* pr = sc.lobe_prob + 3 * (size_t)w.mat;
            const float p0 = pr[0], p1 = pr[1], p2 = pr[2];
            const float u = u01(r.w);
            const float c1 = p0, c2 = p0 + p1;
            lobe = u < c1 ? kLobeDiffuse : (u < c2 ? kLobeSpecular : kLobeTransmit);
            if (lobe == kLobeTransmit && !(p2 > 0.0f)) lobe = p1 > 0.0f ? kLobeSpecular : kLobeDiffuse;
            plobe = lobe == kLobeDiffuse ? p0 : (lobe == kLobeSpecular ? p1 : p2);
            // the listener side pairs a segment with its ARRIVAL vertex: the record of the previous step describes
            // this vertex and learns its lobe now
            if (w.side) store_mat(st, 2u * kp.num_local, w.k - 1, w.slot, w.mat | (lobe << kLobeShift));
        }
        w.lobe = pick ? lobe << kLobeShift : 0u;
        float ox = w.px, oy = w.py, oz = w.pz;
        if (lobe == kLobeDiffuse) {
            // (pre_cone: r.y, r.z, r.w hold cone_local's result for this bounce, computed ahead by another lane — the same operations)
            if (pre_cone) cone_world(w.nx, w.ny, w.nz, __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w), dx, dy, dz);
            else sample_cone(w.nx, w.ny, w.nz, u01(r.y), u01(r.z), kp.cosine, dx, dy, dz);
            float cos_theta = dx * w.nx + dy * w.ny + dz * w.nz;
            float pdf = cos_theta / kPi;
            w.prob_new = pdf * kp.rr_prob;
        } else if (lobe == kLobeSpecular) {                               // mirror direction of the arriving ray
            float dn = ray.dx * w.nx + ray.dy * w.ny + ray.dz * w.nz;
            float k2 = 2.0f * dn;
            dx = fmaf(-k2, w.nx, ray.dx); dy = fmaf(-k2, w.ny, ray.dy); dz = fmaf(-k2, w.nz, ray.dz);
            w.prob_new = kp.rr_prob;
        } else {                                                          // straight on, from the far side of the surface
            dx = ray.dx; dy = ray.dy; dz = ray.dz;
            w.prob_new = kp.rr_prob;
            float back = -2.0f * kp.surface_offset;
            ox = fmaf(back, w.nx, w.px); oy = fmaf(back, w.ny, w.py); oz = fmaf(back, w.nz, w.pz);
        }
        if (pick) w.prob_new = w.prob_new * plobe;
        ray = make_ray(ox, oy, oz, dx, dy, dz);
        return true;
    }
    ray = make_ray(w.px, w.py, w.pz, dx, dy, dz);
    return true;
}

// An end point's collision (the reference's traces query ECC_Pawn too): a sphere; a ray that starts inside
// leaves through the far side.  The legacy tracer's pawn is the same sphere.
__device__ __forceinline__ bool sphere_hit(const Ray& r, const float c[3], float rad, float tmax, float& t_out) {
    float ox = r.ox - c[0], oy = r.oy - c[1], oz = r.oz - c[2];
    float b = fmaf(ox, r.dx, fmaf(oy, r.dy, oz * r.dz));
    float cc = fmaf(ox, ox, fmaf(oy, oy, oz * oz)) - rad * rad;
    float disc = fmaf(b, b, -cc);
    if (!(disc >= 0.0f)) return false;
    float sq = sqrtf(disc);
    float t = -b - sq;
    if (!(t > 0.0f)) t = sq - b;
    if (!(t > 0.0f && t <= tmax)) return false;
    t_out = t;
    return true;
}
// ImpactNormal of a sphere hit: unit (impact - centre), flipped to face the ray origin side like a triangle's
__device__ __forceinline__ void sphere_normal(const Ray& r, float t, const float c[3], float& nx, float& ny, float& nz) {
    float x = fmaf(t, r.dx, r.ox) - c[0], y = fmaf(t, r.dy, r.oy) - c[1], z = fmaf(t, r.dz, r.oz) - c[2];
    float l2 = x * x + y * y + z * z;
    float inv = 1.0f / sqrtf(l2);
    x = x * inv; y = y * inv; z = z * inv;
    float dn = fmaf(x, r.dx, fmaf(y, r.dy, z * r.dz));
    if (dn > 0.0f) { x = -x; y = -y; z = -z; }
    nx = x; ny = y; nz = z;
}

// bottom of the loop (ARTS.cpp:339-347): apply the closest hit (or the miss) and record the segment
// EXT: the instantiation that knows FS_FLAG_DOUBLE_POSITIONS and the end points' collision spheres (both decided at run
// time inside it); the default instantiation carries neither — not a register, not an instruction
// surf (cooperative walk): the hit triangle's unit normal (as stored, not yet flipped) and material bits, handed over by the
// lane that tested it — the loads of hit_surface are saved
template <bool EXT = false>
__device__ __forceinline__ void walker_apply_hit(Walker& w, const KParams& kp, const DeviceScene& sc,
                                                 const SubpathState& st, const Ray& ray, const Trav& T, const float4* surf = nullptr) {
    float qx = w.px, qy = w.py, qz = w.pz;
    double dqx = w.dpx, dqy = w.dpy, dqz = w.dpz;
    uint32_t mat_new = w.mat;
    bool hit = T.leaf_index >= 0;
    float t = T.t;
    if (hit && surf) {
        float x = surf->x, y = surf->y, z = surf->z;
        const float dn = fmaf(x, ray.dx, fmaf(y, ray.dy, z * ray.dz));
        if (dn > 0.0f) { x = -x; y = -y; z = -z; }
        w.nx = x; w.ny = y; w.nz = z;
        mat_new = __float_as_uint(surf->w);
    } else if (hit) hit_surface(sc, T.leaf_index, ray, w.nx, w.ny, w.nz, mat_new);
    // the OTHER end point's collision sphere (the walk's own actor is ignored, ARTS.cpp:322-334); wins ties with a triangle
    const float other_radius = !EXT ? 0.0f : (w.side ? kp.source_radius : kp.listener_radius);
    if (EXT && other_radius > 0.0f) {
        float c[3] = {w.side ? kp.src[0] : kp.lis[0], w.side ? kp.src[1] : kp.lis[1], w.side ? kp.src[2] : kp.lis[2]};
        if (w.side && kp.src_table) {   // batched frame: this pair's source
            const uint32_t sid = w.li / kp.pairs_per_source;
            c[0] = kp.src_table[4 * sid]; c[1] = kp.src_table[4 * sid + 1]; c[2] = kp.src_table[4 * sid + 2];
        }
        float ts;
        if (sphere_hit(ray, c, other_radius, kp.max_trace_dist, ts) && (!hit || ts <= t)) {
            hit = true; t = ts;
            sphere_normal(ray, ts, c, w.nx, w.ny, w.nz);
            mat_new = kNoMat;                                             // a pawn has no UAcousticGeometryComponent
        }
    }
    const bool DPOS = EXT && kp.dpos != 0;
    if (hit) {                                                            // ARTS.cpp:345-347
        if (DPOS) {   // Hit.ImpactPoint + 0.1 * Hit.ImpactNormal in FVector (double) arithmetic; the ray starts at the node's float rounding
            const bool shifted = ray.ox != w.px || ray.oy != w.py || ray.oz != w.pz;   // (transmitted lobe only: never with this flag)
            const double ipx = (shifted ? (double)ray.ox : w.dpx) + (double)t * (double)ray.dx;
            const double ipy = (shifted ? (double)ray.oy : w.dpy) + (double)t * (double)ray.dy;
            const double ipz = (shifted ? (double)ray.oz : w.dpz) + (double)t * (double)ray.dz;
            dqx = ipx + (double)kp.surface_offset * (double)w.nx;
            dqy = ipy + (double)kp.surface_offset * (double)w.ny;
            dqz = ipz + (double)kp.surface_offset * (double)w.nz;
            qx = (float)dqx; qy = (float)dqy; qz = (float)dqz;
        } else {
            qx = fmaf(kp.surface_offset, w.nx, fmaf(t, ray.dx, ray.ox));   // ray origin = node position, except behind
            qy = fmaf(kp.surface_offset, w.ny, fmaf(t, ray.dy, ray.oy));   // the surface for a transmitted segment
            qz = fmaf(kp.surface_offset, w.nz, fmaf(t, ray.dz, ray.oz));
        }
        w.has_normal = true;
    }
    w.arrived = hit;
    // the segment just added (zero length on a miss: the duplicate node of ARTS.cpp:296)
    float nd;
    if (DPOS) {   // FVector::Dist(...) / 1000.f: a double, narrowed by the assignment to float NodeDistance (ARTS.cpp:372-373)
        const double ex = dqx - w.dpx, ey = dqy - w.dpy, ez = dqz - w.dpz;
        nd = (float)(sqrt(ex * ex + ey * ey + ez * ez) / (double)kp.dist_divisor);
    } else {
        float ddx = qx - w.px, ddy = qy - w.py, ddz = qz - w.pz;
        float dist = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);            // ARTS.cpp:372
        nd = dist / kp.dist_divisor;                                      // ARTS.cpp:373
    }
    // Record for EvaluatePath (done by connect_kernel in path order): node i of the reference's loop is
    // the DEPARTURE node on the source side and — the listener subpath being reversed in the connected
    // path — the ARRIVAL node on the listener side.
    const float2 rec_np = w.side == 0 ? make_float2(nd, w.prob) : make_float2(nd, w.prob_new);
    const uint32_t rec_mat = w.side == 0 ? (w.mat | w.lobe) : mat_new;   // w.lobe: 0 unless FS_FLAG_MATERIAL_LOBES picked one here
    if (rec_in_main(st, w.k)) {
        const size_t r = rec_main(2u * kp.num_local, w.k, w.slot);       // consecutive lanes, consecutive words
        st.seg_np[r] = rec_np;
        st.seg_mat[r] = rec_mat;
        if (st.seg_pos) st.seg_pos[r] = make_float4(qx, qy, qz, 0.0f);   // all-connections mode (wave-uniform)
        if (st.seg_nrm) st.seg_nrm[r] = make_float4(w.nx, w.ny, w.nz, 0.0f);   // balance-heuristic weights only
    } else if (rec_fits(st, w.k, w.slot)) {                              // depth = 0: step 65.. of one of the longest walks
        const size_t r = rec_over(st, w.k, w.slot);
        st.over_np[r] = rec_np;
        st.over_mat[r] = rec_mat;
        if (st.seg_pos) st.over_pos[r] = make_float4(qx, qy, qz, 0.0f);
        if (st.seg_nrm) st.over_nrm[r] = make_float4(w.nx, w.ny, w.nz, 0.0f);
    } else {
        *st.overflow = 1u;                                               // the host grows the tier and traces again
    }
    w.px = qx; w.py = qy; w.pz = qz;
    if (DPOS) { w.dpx = dqx; w.dpy = dqy; w.dpz = dqz; }
    w.mat = mat_new;
    w.prob = w.prob_new;
    ++w.k;
}

// staged walks: leave / pick up a walk between two stages (SubpathState::cont_a / cont_b)
__device__ __forceinline__ void walker_suspend(const Walker& w, const SubpathState& st) {
    st.cont_a[w.slot] = make_float4(w.px, w.py, w.pz, w.prob);
    st.cont_b[w.slot] = make_float4(w.nx, w.ny, w.nz, __uint_as_float((w.mat & 0xFFFFu) | (w.has_normal ? kContHasNormal : 0u) |
                                                                        (w.arrived ? kContArrived : 0u) | kContAlive));
}
__device__ __forceinline__ bool walker_resume(Walker& w, const SubpathState& st, int step) {   // false: the walk has ended before
    const float4 a = st.cont_a[w.slot], c = st.cont_b[w.slot];
    const uint32_t bits = __float_as_uint(c.w);
    if (!(bits & kContAlive)) return false;
    w.px = a.x; w.py = a.y; w.pz = a.z; w.prob = a.w; w.prob_new = a.w;
    w.nx = c.x; w.ny = c.y; w.nz = c.z;
    w.mat = bits & 0xFFFFu;
    w.has_normal = (bits & kContHasNormal) != 0u;
    w.arrived = (bits & kContArrived) != 0u;
    w.k = step;
    return true;
}
// slots a stage covers: the walks the previous stage suspended at step stage.begin, i.e. those of stage.begin steps or
// more (one of exactly that length ends at its first roulette here) — buckets begin .. FS_MAX_DEPTH of the length-sorted
// schedule (the last bucket holds every walk of FS_MAX_DEPTH steps or more: a stage that starts later than that visits
// them all and the continuation record says which still walk: a walk of that bucket that ENDS — in whatever stage, also one that
// began before FS_MAX_DEPTH — clears its record; round 3 cleared it only in stages that begin at FS_MAX_DEPTH or later, so
// that a walk of 64 .. 69 steps under bounds like 9, 70 kept the record of its suspension at step 9 and walked on from it)
__device__ __forceinline__ uint32_t stage_slots(const WalkStage& sr, const SubpathState& st, uint32_t total, const unsigned* s_cnt) {
    if (sr.begin <= 0) return total;
    uint32_t n = 0;
    for (int L = min(sr.begin, FS_MAX_DEPTH); L <= FS_MAX_DEPTH; ++L) n += s_cnt[L];
    if (n > sr.slots_cap) { *st.overflow = 1u; n = sr.slots_cap; }   // more long walks than the launch has lanes for: the frame is traced again
    return n;
}

// slots of the long-walk lane (WalkLane): the walks of len steps or more, at most cap — the same number in every
// part of every launch of the frame (a function of the plan pass's bucket counts alone)
__device__ __forceinline__ uint32_t lane_slots(const WalkLane& ln, const unsigned* s_cnt) {
    if (ln.len <= 0) return 0u;
    uint32_t n = 0;
    for (int L = min(ln.len, FS_MAX_DEPTH); L <= FS_MAX_DEPTH; ++L) n += s_cnt[L];
    return min(n, ln.cap);
}

template <bool EXT = false>
__device__ __forceinline__ void walker_finish(const Walker& w, const SubpathState& st) {
    if (EXT && st.end_posd) { st.end_posd[3 * (size_t)w.slot] = w.dpx; st.end_posd[3 * (size_t)w.slot + 1] = w.dpy; st.end_posd[3 * (size_t)w.slot + 2] = w.dpz; }
    st.end_pos[w.slot] = make_float4(w.px, w.py, w.pz, w.prob);
    st.end_misc[w.slot] = make_uint2(w.mat, (uint32_t)w.k);
}

// ---------------------------------------------------------------------------------------------------
// plan_kernel: the number of segments a subpath takes under Russian roulette depends only on the RNG
// stream (seed, pair, side, bounce) — never on the geometry — so it is known before any ray is traced.
// One pass buckets the subpath indices by length: bucket L owns perm[L * total, L * total + count[L])
// (worst-case capacity, so no prefix pass is needed); workgroups reserve their share of a bucket with one
// atomicAdd per occupied length.  Walk lanes then read the buckets in DESCENDING length order, so every
// wave holds walks of equal length and no lane idles because its neighbours' walks ended earlier.
// (Order never affects results.)  The pass also performs FlushEnergyBuffer (ARTS.cpp:157-161).
//   scratch[0] = subpath queue head (persistent walk), [1, 1 + kPlanBuckets) = bucket counts.
// ---------------------------------------------------------------------------------------------------
constexpr int kPlanBuckets = FS_MAX_DEPTH + 1;
constexpr int kPlanItems = 4;   // subpaths per plan-kernel thread

__device__ __forceinline__ int planned_length(uint32_t g, const KParams& kp) {
    const uint32_t n = kp.num_local;
    const uint32_t side = g >= n ? 1u : 0u;
    const uint32_t li = g - side * n, sid = li / kp.pairs_per_source;
    const uint32_t pair = kp.pair_begin + (li - sid * kp.pairs_per_source);       // batched frame: per-source pair index
    const uint32_t seed = item_seed_lo(kp, sid);
    int k = 0;
    for (; k < kp.depth; ++k) {
        const uint4 r = philox(pair, ((uint32_t)k << 1) | side, 0, seed, kp.seed_hi);
        if (!(u01(r.x) < kp.rr_prob)) break;   // ARTS.cpp:300-301
    }
    return k;
}

__device__ __forceinline__ void plan_body(const uint32_t bid, const uint32_t nblocks, const KParams& kp,
                                          unsigned* __restrict__ scratch, uint32_t* __restrict__ perm,
                                          float* __restrict__ energy, const int energy_words,
                                          float* const* __restrict__ energy_tab, const int energy_count) {
    __shared__ unsigned s_hist[kPlanBuckets];
    __shared__ unsigned s_base[kPlanBuckets];
    __shared__ unsigned s_seg;
    if (threadIdx.x == 0) s_seg = 0u;
    for (int i = threadIdx.x; i < kPlanBuckets; i += kBlock) s_hist[i] = 0u;
    if (energy_tab) {   // batched frame: every source's buffer (the table was copied on this stream before the launch)
        for (int k = 0; k < energy_count; ++k) {
            float* e = energy_tab[k];
            for (int i = bid * kBlock + threadIdx.x; i < energy_words; i += nblocks * kBlock) e[i] = 0.0f;
        }
    } else {
        for (int i = bid * kBlock + threadIdx.x; i < energy_words; i += nblocks * kBlock) energy[i] = 0.0f;
    }
    __syncthreads();
    const uint32_t total = 2u * kp.num_local;
    // kPlanItems subpaths per thread: the bucket counters are a handful of hot addresses, and every workgroup
    // pays one global atomic per occupied length — fewer, larger workgroup batches mean fewer of them
    int L[kPlanItems];   // bucket = planned length, walks of more than FS_MAX_DEPTH steps (depth = 0 only) share the last one
    unsigned rank[kPlanItems];
    unsigned my_segments = 0;
#pragma unroll
    for (int it = 0; it < kPlanItems; ++it) {
        const uint32_t g = (bid * kPlanItems + it) * kBlock + threadIdx.x;
        L[it] = 0; rank[it] = 0;
        if (g < total) {
            const int len = planned_length(g, kp);
            my_segments += (unsigned)len;
            L[it] = min(len, FS_MAX_DEPTH);
            rank[it] = atomicAdd(&s_hist[L[it]], 1u);
        }
    }
    if (my_segments) atomicAdd(&s_seg, my_segments);
    __syncthreads();
    for (int i = threadIdx.x; i < kPlanBuckets; i += kBlock)
        if (s_hist[i]) s_base[i] = atomicAdd(&scratch[1 + i], s_hist[i]);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kPlanItems; ++it) {
        const uint32_t g = (bid * kPlanItems + it) * kBlock + threadIdx.x;
        if (perm && g < total) perm[(size_t)L[it] * total + s_base[L[it]] + rank[it]] = g;
    }
    // work counter: walk segments of this frame (a walk of length L traces L rays), one atomic per workgroup
    if (threadIdx.x == 0 && s_seg) atomicAdd(reinterpret_cast<unsigned long long*>(scratch + kCounterWord) + 7, (unsigned long long)s_seg);   // fs_stats.planned_segments
}


// The same pass for SMALL frames (at most kPlanCoopMax subpaths) and for uncapped walks somebody waits for (at most
// kPlanCoopMaxUncapped: KParams.plan_coop, set by frame_describe): the roulette of one subpath is a serial chain of Philox
// evaluations — up to ~85 for the longest of 2 000 uncapped walks, 42 us with a subpath per thread, a tenth of the reference's
// tick — but its bounces are independent: a wave takes plan_coop_items() subpaths and evaluates 64 bounces of one at a time,
// lane j the roulette of bounce j; the first lane whose draw ends the walk gives its length (ballot + find-first).  (64 draws
// per subpath where the chain makes 10 on average: for capped walks of a chip-filling frame the chain is the cheaper one.)
// subpaths per wave: 8 for the reference's own frame (2 000 subpaths: 250 waves), more for the ticks of many sources — every
// workgroup adds its counts to the ~ 30 occupied length buckets with one global atomic each, and with 32 subpaths per workgroup
// those atomics (40 000 on 65 addresses at 64 000 subpaths) were the pass: 34 us
__host__ __device__ inline int plan_coop_items(uint32_t lanes) { return lanes <= 4096u ? 8 : (lanes <= 32768u ? 16 : 32); }
__device__ __forceinline__ void plan_coop_body(const uint32_t bid, const uint32_t nblocks, const KParams& kp,
                                               unsigned* __restrict__ scratch, uint32_t* __restrict__ perm,
                                               float* __restrict__ energy, const int energy_words,
                                               float* const* __restrict__ energy_tab, const int energy_count) {
    __shared__ unsigned s_hist[kPlanBuckets];
    __shared__ unsigned s_base[kPlanBuckets];
    __shared__ unsigned s_seg;
    if (threadIdx.x == 0) s_seg = 0u;
    for (int i = threadIdx.x; i < kPlanBuckets; i += kBlock) s_hist[i] = 0u;
    if (energy_tab) {
        for (int k = 0; k < energy_count; ++k) {
            float* e = energy_tab[k];
            for (int i = bid * kBlock + threadIdx.x; i < energy_words; i += nblocks * kBlock) e[i] = 0.0f;
        }
    } else {
        for (int i = bid * kBlock + threadIdx.x; i < energy_words; i += nblocks * kBlock) energy[i] = 0.0f;
    }
    __syncthreads();
    const uint32_t total = 2u * kp.num_local, n = kp.num_local;
    const uint32_t lane = threadIdx.x & 63u;
    const int items = plan_coop_items(total);
    const uint32_t first = (bid * (kBlock / 64) + (threadIdx.x >> 6)) * (uint32_t)items;   // this wave's subpaths [first, first + items)
    int my_len = 0;
    for (int it = 0; it < items; ++it) {                     // (wave-uniform)
        const uint32_t g = first + (uint32_t)it;
        if (g >= total) break;
        const uint32_t side = g >= n ? 1u : 0u;
        const uint32_t li = g - side * n, sid = li / kp.pairs_per_source;
        const uint32_t pair = kp.pair_begin + (li - sid * kp.pairs_per_source);
        const uint32_t seed = item_seed_lo(kp, sid);
        int len = kp.depth;
        for (int k0 = 0; k0 < kp.depth; k0 += 64) {
            const int k = k0 + (int)lane;
            bool ends = k >= kp.depth;
            if (!ends) {
                const uint4 r = philox(pair, ((uint32_t)k << 1) | side, 0, seed, kp.seed_hi);
                ends = !(u01(r.x) < kp.rr_prob);              // ARTS.cpp:300-301
            }
            const unsigned long long m = __ballot(ends);
            if (m != 0ull) { len = k0 + __ffsll((long long)m) - 1; break; }
        }
        if (lane == (uint32_t)it) my_len = len;
    }
    const bool mine = lane < (uint32_t)items && first + lane < total;
    const int L = min(my_len, FS_MAX_DEPTH);
    unsigned rank = 0;
    if (mine) {
        rank = atomicAdd(&s_hist[L], 1u);
        if (my_len) atomicAdd(&s_seg, (unsigned)my_len);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kPlanBuckets; i += kBlock)
        if (s_hist[i]) s_base[i] = atomicAdd(&scratch[1 + i], s_hist[i]);
    __syncthreads();
    if (mine && perm) perm[(size_t)L * total + s_base[L] + rank] = first + lane;
    if (threadIdx.x == 0 && s_seg) atomicAdd(reinterpret_cast<unsigned long long*>(scratch + kCounterWord) + 7, (unsigned long long)s_seg);   // fs_stats.planned_segments
}

// launch slot -> subpath index through the buckets, longest walks first.  s_cnt = bucket counts in LDS.
__device__ __forceinline__ uint32_t planned_subpath(uint32_t slot, int depth, uint32_t total, const unsigned* s_cnt,
                                                    const uint32_t* __restrict__ perm) {
    uint32_t acc = 0;
    for (int L = depth; L > 0; --L) {
        const uint32_t c = s_cnt[L];
        if (slot < acc + c) return perm[(size_t)L * total + (slot - acc)];
        acc += c;
    }
    return perm[slot - acc];   // bucket 0
}


// IGN (= EXT unless said otherwise): the queries skip the triangles of the actor the walk starts from; the fused frame kernel's
// EXT flavour asks for that alone (IGN without EXT: no double positions, no end-point spheres — 23 -> 64 spilled registers with them)
template <int LOBES, bool COUNT, bool EXT = false, bool IGN = EXT>
__device__ __forceinline__ void walk_shared_body(const uint32_t bid, const DeviceScene& sc, const KParams& kp,
                                                 const SubpathState& st, const unsigned* __restrict__ scratch,
                                                 const uint32_t* __restrict__ perm, const WalkStage sr = WalkStage()) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] | work-sharing area
    int* s_stack = s_dyn;
    __shared__ unsigned s_cnt[kPlanBuckets];
    if (perm) {
        for (int i = threadIdx.x; i <= FS_MAX_DEPTH; i += kBlock) s_cnt[i] = i <= min(kp.depth, FS_MAX_DEPTH) ? scratch[1 + i] : 0u;
    }
    if (perm) __syncthreads();
    const uint32_t li = bid * kBlock + threadIdx.x;
    if (li >= stage_slots(sr, st, 2u * kp.num_local, s_cnt)) return;
    const uint32_t slot = li;
    const uint32_t g = perm ? planned_subpath(slot, min(kp.depth, FS_MAX_DEPTH), 2u * kp.num_local, s_cnt, perm) : slot;
    int* stack = &s_stack[threadIdx.x];
    Walker w;
    walker_start(w, g, slot, kp, st, sr.begin == 0);
    if (sr.begin > 0 && !walker_resume(w, st, sr.begin)) return;
    Ray ray;
    uint32_t cnt_nv = 0u, cnt_nt = 0u, cnt_ni = 0u, cnt_nl = 0u, cnt_nd = 0u;
#ifdef FS_WAVE_TIMELINE
    const unsigned long long tl_r0 = __builtin_amdgcn_s_memrealtime(), tl_c0 = __builtin_amdgcn_s_memtime();
    unsigned long long tl_trav = 0, tl_seg = 0;
#endif
    while (true) {
        if (w.k >= sr.end) { walker_suspend(w, st); break; }          // staged walk: the next stage goes on from here
        if (!walker_next_ray<LOBES>(w, kp, sc, st, ray)) {
            walker_finish<EXT>(w, st);
            if (st.cont_b && w.k >= FS_MAX_DEPTH) st.cont_b[slot] = make_float4(0.f, 0.f, 0.f, 0.f);   // a walk of the last schedule bucket: later stages visit this slot again
            break;
        }
        Trav T;
#ifdef FS_WAVE_TIMELINE
        const unsigned long long tl_a = __builtin_amdgcn_s_memtime();
#endif
        trav_run_shared<COUNT, IGN>(sc, ray, T, stack, s_dyn, kp.max_trace_dist, true, w.ign);   // (IGN: the walk's own actor is ignored)
#ifdef FS_WAVE_TIMELINE
        tl_trav += __builtin_amdgcn_s_memtime() - tl_a;
        ++tl_seg;
#endif
        if (COUNT) { cnt_nv += T.nv; cnt_nt += T.nt; cnt_ni += T.ni; cnt_nl += T.nl; cnt_nd += T.nd; }
        walker_apply_hit<EXT>(w, kp, sc, st, ray, T);
    }
    if (COUNT) {
        add_fetch_counts(const_cast<unsigned*>(scratch), 3, cnt_nv, cnt_nt);
        unsigned long long* counters = reinterpret_cast<unsigned long long*>(const_cast<unsigned*>(scratch) + kCounterWord);
        if (cnt_ni) { atomicAdd(&counters[8], (unsigned long long)cnt_ni); atomicAdd(&counters[9], (unsigned long long)cnt_nl); atomicAdd(&counters[10], (unsigned long long)cnt_nd); }
    }
#ifdef FS_WAVE_TIMELINE
    {
        unsigned long long seg_max = tl_seg, trav_max = tl_trav;   // lanes of a wave leave the loop at different bounces
        for (int o = 32; o > 0; o >>= 1) {
            seg_max = max(seg_max, (unsigned long long)__shfl_xor((long long)seg_max, o));
            trav_max = max(trav_max, (unsigned long long)__shfl_xor((long long)trav_max, o));
        }
        if ((threadIdx.x & 63u) == 0u && g_wave_buf) {
            unsigned long long* o = g_wave_buf + 8ull * (bid * (kBlock / 64) + (threadIdx.x >> 6));
            o[0] = tl_r0; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = trav_max;
            o[3] = __builtin_amdgcn_s_memtime() - tl_c0; o[4] = 0; o[5] = seg_max;
            o[6] = __builtin_amdgcn_s_getreg(((8 - 1) << 11) | (0 << 6) | 4)            // HW_REG_HW_ID bits [7:0]
                   | ((unsigned long long)__builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20) << 32);   // HW_REG_XCC_ID
            o[7] = slot;
        }
    }
#endif
}


// Small frames on sparse waves: a frame of a few thousand subpaths is a handful of waves and takes the latency of
// its longest chain of closest-hit queries.  Here a wave owns only `rays_per_wave` subpaths (its first lanes) and
// the other lanes help with every query — the legacy tracer's scheme (update_sound_shared_kernel).  The loop is
// wave-uniform: lanes whose walk has ended (or that never had one) keep calling the shared traversal as helpers.
template <int LOBES, bool COUNT, bool EXT = false, bool IGN = EXT>
__device__ __forceinline__ void walk_sparse_body(const uint32_t bid, const DeviceScene& sc, const KParams& kp,
                                                 const SubpathState& st, const unsigned* __restrict__ scratch,
                                                 const uint32_t* __restrict__ perm, const int rays_per_wave,
                                                 const WalkStage sr = WalkStage(), const WalkLane ln = WalkLane()) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] | work-sharing area
    int* s_stack = s_dyn;
    __shared__ unsigned s_cnt[kPlanBuckets];
    if (perm) {
        for (int i = threadIdx.x; i <= min(kp.depth, FS_MAX_DEPTH); i += kBlock) s_cnt[i] = scratch[1 + i];
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = bid * (kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t slot = wave * (uint32_t)rays_per_wave + lane;
    bool alive = lane < (uint32_t)rays_per_wave && slot < stage_slots(sr, st, 2u * kp.num_local, s_cnt);
    if (ln.len > 0 && ln.mode == kLaneSkip) alive = alive && slot >= lane_slots(ln, s_cnt);   // (the long-walk lane's slots: cooperative waves of the same launch)
    int* stack = &s_stack[threadIdx.x];
    Walker w;
    walker_start(w, alive ? (perm ? planned_subpath(slot, min(kp.depth, FS_MAX_DEPTH), 2u * kp.num_local, s_cnt, perm) : slot) : 0u,
                 slot, kp, st, alive && sr.begin == 0);
    if (alive && sr.begin > 0) alive = walker_resume(w, st, sr.begin);
    Ray ray;
    uint32_t cnt_nv = 0u, cnt_nt = 0u;
    while (true) {
        bool go = false;
        if (alive) {
            if (w.k >= sr.end) { walker_suspend(w, st); alive = false; }   // staged walk: the next stage goes on from here
            else {
                go = walker_next_ray<LOBES>(w, kp, sc, st, ray);
                if (!go) {
                    walker_finish<EXT>(w, st);
                    if (st.cont_b && w.k >= FS_MAX_DEPTH) st.cont_b[slot] = make_float4(0.f, 0.f, 0.f, 0.f);   // a walk of the last schedule bucket: later stages visit this slot again
                    alive = false;
                }
            }
        }
        if (__ballot(go) == 0ull) break;
        Trav T;
        trav_run_shared<COUNT, IGN>(sc, ray, T, stack, s_dyn, kp.max_trace_dist, go, w.ign);
        if (COUNT) { cnt_nv += T.nv; cnt_nt += T.nt; }
        if (go) walker_apply_hit<EXT>(w, kp, sc, st, ray, T);
    }
    if (COUNT) add_fetch_counts(const_cast<unsigned*>(scratch), 3, cnt_nv, cnt_nt);
}

}  // namespace
}  // namespace fs
