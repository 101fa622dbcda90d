// fs_dev_connect.hpp — the connect pass: ConnectSubpaths + EvaluatePath + clamp / gain + deposit (connect_body).
#pragma once
#include "fs_dev_walk.hpp"

namespace fs {
namespace {

// ---------------------------------------------------------------------------------------------------
// source directivity (fs_source_set_directivity, include/frequensee.h): one more factor per band on every deposit of a path,
// D_b(theta) of the direction w_e the path left the source in.  The factor comes after the clamp of EvaluatePath
// (e = min(E_b, clamp) * gain * norm [* MIS weight] * D_b): the reference's EvaluatePath stays as it is and the result is
// linear in the table.  Nothing of the walk changes — no sample, no RNG word, no MIS weight (the pattern is part of the
// contribution, not of the sampling density).
// ---------------------------------------------------------------------------------------------------
// The step with which the source's walk left the source: its first record with a length.  Until a ray hits, the walk stays
// where it is and records a zero-length segment (walker_apply_hit: the duplicate node of ARTS.cpp:296).  -1: never left.
__device__ __forceinline__ int emission_step(const SubpathState& st, uint32_t total, uint32_t sf, int records) {
    for (int j = 0; j < records; ++j)
        if (load_np(st, total, j, sf).x != 0.0f) return j;
    return -1;
}
// ... and the ray it traced then: the sphere sample walker_next_ray drew for that step (source side, no normal yet), from the
// same Philox words — the pair's global RNG index and the item's seed word, so the direction does not depend on sharding
__device__ __forceinline__ void emission_ray(const KParams& kp, uint32_t li, int step, float& wx, float& wy, float& wz) {
    const uint32_t sid = li / kp.pairs_per_source;
    const uint32_t pair = kp.pair_begin + (li - sid * kp.pairs_per_source);
    const uint32_t seed = kp.item_seeds > 0 ? item_seed_lo(kp, sid) : kp.seed_lo;
    const uint32_t bs = (uint32_t)step << 1;
    const uint4 r = philox(pair, bs, 0, seed, kp.seed_hi);
    sample_sphere(pair, bs, r, seed, kp.seed_hi, wx, wy, wz);
}
// Order window (fs_source_set_order_window): the order of a path is the number of its nodes that a walk step's HIT made.  A
// step that misses leaves the walk where it is: its record has the length 0 exactly (q = p above, sqrtf(0) / divisor).  A
// step that hits moves the node by t d + offset n with n . d <= 0: squared length t^2 + offset^2 + 2 t offset (n . d) >=
// (t - offset)^2, zero only for a ray that meets a surface head-on (d = -n in every bit) at exactly t = offset — see DESIGN.md
// section 8, "Order window".  So the records tell the hits apart, as emission_step above reads them.
__device__ __forceinline__ int order_hit(float nd) { return nd != 0.0f ? 1 : 0; }
// theta = atan2f(|w x f|, w . f) (well-conditioned near 0 and pi, unlike acosf of the dot); x = theta (K - 1) / pi,
// k = min((int)x, K - 2), t = x - k.  (A zero-length connection of a walk that never left has no direction: theta = 0.)
struct DirLookup { const float* row; int K, k; float t; };
__device__ __forceinline__ DirLookup dir_lookup(const Directivity& d, float wx, float wy, float wz) {
    DirLookup L;
    L.row = d.table; L.K = d.samples; L.k = 0; L.t = 0.0f;
    if (!d.table) return L;
    const float fx = d.fwd[0], fy = d.fwd[1], fz = d.fwd[2];
    const float cx = wy * fz - wz * fy, cy = wz * fx - wx * fz, cz = wx * fy - wy * fx;
    const float sn = sqrtf(cx * cx + cy * cy + cz * cz), cs = wx * fx + wy * fy + wz * fz;
    float x = atan2f(sn, cs) * (float)(d.samples - 1) / kPi;
    if (!(x >= 0.0f)) x = 0.0f;
    L.k = min((int)x, d.samples - 2);
    L.t = x - (float)L.k;
    return L;
}
// D_b = T[b][k] + t (T[b][k+1] - T[b][k]): a constant table gives that constant exactly.  Plain loads: at most 5.8 KB per
// source, cache-resident (no LDS: the connect part's occupancy stays as it is)
__device__ __forceinline__ float dir_gain(const DirLookup& L, int b) {
    if (!L.row) return 1.0f;
    const float* r = L.row + (size_t)b * (size_t)L.K + (size_t)L.k;
    const float t0 = r[0], t1 = r[1];
    return t0 + L.t * (t1 - t0);
}

// ---------------------------------------------------------------------------------------------------
// connect_kernel: ConnectSubpaths + EvaluatePath + clamp/gain + deposit
// ---------------------------------------------------------------------------------------------------
// pairs_per_wave < 64: sparse waves for small frames — a wave owns that many pairs (its first lanes), the other
// lanes only help with the shared visibility queries (a frame of a few thousand pairs is otherwise a few waves
// waiting for their longest traversal).
// BATCH: a batched frame (fs_compute_energy_response_batch): the pairs of several sources lie end to end
// (kp.pairs_per_source each) and every source has its own energy buffer (energy_tab / fixed_tab); a workgroup
// takes (source, chunk) items and flushes its LDS histogram whenever the source changes.
// AHEAD (the connect kernels of uncapped walks that are waited for): a lane that evaluates its pair's path alone requests the
// records of AHEAD segments at once and applies them in path order — the same operations in the same order.  The records of a
// walk lie a whole level apart ([step][slot]): one at a time, every segment of a 100-segment path waited for its own miss.
// (Also measured: the paths of 40 segments or more evaluated by the whole wave, as a sparse wave does for every path — no gain
// on top of this: 88 -> 92 us at cfg3's size.  With the records ahead the longest path is no longer what the pass waits for.)
// DIR (connect_dir_kernel only): the source's directivity, `dir` — the pair's own lane weights its deposits by D_b(w_e) —
// and its order window: the evaluation counts the records a hit made, a path outside [min_order, max_order] deposits nothing.
template <int B, int LOBES, bool BATCH, bool COUNT, bool EXT = false, int AHEAD = 1, bool DIR = false>
__device__ __forceinline__ void connect_body(const uint32_t bid, const uint32_t nblocks, const DeviceScene& sc,
                                             const KParams& kp, const SubpathState& st, float* __restrict__ energy,
                                             unsigned long long* __restrict__ fixed, unsigned* queue_head,
                                             const int pairs_per_wave, float* const* __restrict__ energy_tab,
                                             unsigned long long* const* __restrict__ fixed_tab, const DirArgs& dir = DirArgs()) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] stack | [B][hist_window] histogram
    int* s_stack = s_dyn;
    float* s_hist = reinterpret_cast<float*>(s_dyn + (size_t)sc.stack_rows * kBlock);
    const int nb = kp.num_bins, W = kp.hist_window, NB = band_count<B>(kp);   // LDS histogram = the first W bins of every band (see KParams)
    int* s_share = reinterpret_cast<int*>(s_hist + (size_t)NB * W);   // work-sharing area of trav_any_shared
    __shared__ int s_lo, s_hi;
    __shared__ unsigned s_dep, s_tst, s_sgs;
#ifdef FS_WAVE_TIMELINE
    unsigned long long tl[6] = {__builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0, 0};
#endif
    for (int i = threadIdx.x; i < NB * W; i += kBlock) s_hist[i] = 0.0f;
    if (threadIdx.x == 0) { s_lo = nb; s_hi = -1; s_dep = 0u; s_tst = 0u; s_sgs = 0u; }
    // this frame's walk is over: rearm the frame scratch (queue head, plan counts and cursors) for the next one
    if (bid == 0u)
        for (int i = threadIdx.x; i < 1 + 2 * kPlanBuckets; i += kBlock) queue_head[i] = 0u;
    __syncthreads();

    const uint32_t n = kp.num_local;
    const uint32_t total = 2u * n;
    unsigned my_deposits = 0, my_tested = 0, my_segments = 0;
    uint32_t cnt_nv = 0u, cnt_nt = 0u;
    // whole workgroups step through the pairs: every lane of a wave takes part in the shared visibility queries,
    // also the ones without a pair or without a segment to test
    const uint32_t ppw = (uint32_t)pairs_per_wave, per_block = ppw * (kBlock / 64);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    // one chunk of per_block pairs [first, first + per_block) clipped to `end`, deposits into s_hist / fixed_dst
    auto chunk = [&](uint32_t first, uint32_t end, unsigned long long* fixed_dst, float* far_dst) {
        const uint32_t li = first + wave * ppw + lane;
        const bool active = lane < ppw && li < end;
        const uint32_t lc = active ? li : 0u;
        const uint32_t sf = slot_of(st, lc), sl = slot_of(st, n + lc);   // where the walk left the two subpaths of the pair
        const float4 F = st.end_pos[sf];
        const uint2 Fm = st.end_misc[sf];
        const float4 L = st.end_pos[sl];
        const uint2 Lm = st.end_misc[sl];
        // visibility F_k -> B_m - 0.1 * unit(B_m - F_k) (ARTS.cpp:252-254); visible iff NO hit
        float dx = L.x - F.x, dy = L.y - F.y, dz = L.z - F.z;
        float l2 = dx * dx + dy * dy + dz * dz;
        float len = sqrtf(l2);
        float inv = 1.0f / len;
        float tmax = len - kp.connect_pullback;
        float ux = dx * inv, uy = dy * inv, uz = dz * inv;
        float conn_nd = 0.0f;       // FS_FLAG_DOUBLE_POSITIONS: the connection segment's scaled length, from the double end points
        if (EXT && kp.dpos) {       // (wave-uniform) FVector end points: difference, length and unit direction in double
            const double* Fd = st.end_posd + 3 * (size_t)sf;
            const double* Ld = st.end_posd + 3 * (size_t)sl;
            const double ex = Ld[0] - Fd[0], ey = Ld[1] - Fd[1], ez = Ld[2] - Fd[2];
            const double e2 = ex * ex + ey * ey + ez * ez;
            const double elen = sqrt(e2), einv = 1.0 / elen;
            l2 = e2 > 1e-8f ? 1.0f : 0.0f;                       // only its comparison with 1e-8 is used below
            ux = (float)(ex * einv); uy = (float)(ey * einv); uz = (float)(ez * einv);
            tmax = (float)(elen - kp.connect_pullback);
            conn_nd = (float)(elen / (double)kp.dist_divisor);
        }
        bool has_ray = active && (l2 > 1e-8f) && (tmax > 0.0f);
        Ray ray = make_ray(F.x, F.y, F.z, ux, uy, uz);
        // ConnectSubpaths ignores no actor (ARTS.cpp:252-254): the end points' collision spheres block
        bool sphere_blocked = false;
        if (EXT && has_ray && (kp.listener_radius > 0.0f || kp.source_radius > 0.0f)) {
            float ts;
            if (kp.listener_radius > 0.0f && sphere_hit(ray, kp.lis, kp.listener_radius, tmax, ts)) sphere_blocked = true;
            if (kp.source_radius > 0.0f) {
                float c[3] = {kp.src[0], kp.src[1], kp.src[2]};
                if (kp.src_table) { const uint32_t sid = lc / kp.pairs_per_source; c[0] = kp.src_table[4 * sid]; c[1] = kp.src_table[4 * sid + 1]; c[2] = kp.src_table[4 * sid + 2]; }
                if (sphere_hit(ray, c, kp.source_radius, tmax, ts)) sphere_blocked = true;
            }
            if (sphere_blocked) has_ray = false;   // settled without a traversal
        }
#ifdef FS_WAVE_TIMELINE
        if (!tl[1]) tl[1] = __builtin_amdgcn_s_memrealtime();   // first chunk: set-up and end-state loads done
#endif
        my_tested += active ? 1u : 0u;                                // one ConnectSubpaths per pair (ARTS.cpp:232 counts the connected ones)
        my_segments += active ? Fm.y + Lm.y : 0u;                     // the steps the two walks TOOK (each wrote its own count with its end state)
        const bool hit = trav_any_shared<COUNT>(sc, has_ray, ray, tmax, &s_stack[threadIdx.x], s_share, &cnt_nv, &cnt_nt);
#ifdef FS_WAVE_TIMELINE
        if (!tl[2]) tl[2] = __builtin_amdgcn_s_memrealtime();   // first chunk: visibility queries done
#endif
        float E[Bands<B>::kMax];
#pragma unroll
        for (int b = 0; b < Bands<B>::kMax; ++b) E[b] = 1.0f;
        float sd = 0.0f;
        [[maybe_unused]] int order = 0;   // DIR: the path's nodes that a hit made (see order_hit)
        // one lane evaluates its pair's connected path alone: EvaluatePath over F0..Fk, Bm..B0 (ARTS.cpp:262-267, 360-420), in path order
        auto eval_alone = [&]() {
        const int kf = (int)Fm.y, kl = (int)Lm.y;
        if (AHEAD > 1) {
            for (int j0 = 0; j0 < kf; j0 += AHEAD) {                      // source-side segments F_j -> F_j+1, AHEAD records in flight
                float2 np[AHEAD];
                uint32_t mt[AHEAD];
#pragma unroll
                for (int u = 0; u < AHEAD; ++u) { const int j = min(j0 + u, kf - 1); np[u] = load_np(st, total, j, sf); mt[u] = load_mat(st, total, j, sf); }
#pragma unroll
                for (int u = 0; u < AHEAD; ++u)
                    if (j0 + u < kf) { sd += np[u].x; if (DIR) order += order_hit(np[u].x); apply_segment<B, LOBES>(E, np[u].x, mt[u], np[u].y, kp, sc); }
            }
        } else
        for (int j = 0; j < kf; ++j) {                                // source-side segments F_j -> F_j+1
            const float2 np = load_np(st, total, j, sf);
            sd += np.x;                                               // ARTS.cpp:374
            if (DIR) order += order_hit(np.x);
            apply_segment<B, LOBES>(E, np.x, load_mat(st, total, j, sf), np.y, kp, sc);
        }
        {                                                             // connection segment: F_k's material/prob
            float dist = sqrtf(l2);
            float nd = (EXT && kp.dpos) ? conn_nd : dist / kp.dist_divisor;
            sd += nd;
            apply_segment<B, LOBES>(E, nd, Fm.x, F.w, kp, sc);
        }
        if (AHEAD > 1) {
            for (int j0 = kl - 1; j0 >= 0; j0 -= AHEAD) {                 // listener-side segments B_j+1 -> B_j
                float2 np[AHEAD];
                uint32_t mt[AHEAD];
#pragma unroll
                for (int u = 0; u < AHEAD; ++u) { const int j = max(j0 - u, 0); np[u] = load_np(st, total, j, sl); mt[u] = load_mat(st, total, j, sl); }
#pragma unroll
                for (int u = 0; u < AHEAD; ++u)
                    if (j0 - u >= 0) { sd += np[u].x; if (DIR) order += order_hit(np[u].x); apply_segment<B, LOBES>(E, np[u].x, mt[u], np[u].y, kp, sc); }
            }
        } else
        for (int j = kl - 1; j >= 0; --j) {                           // listener-side segments B_j+1 -> B_j
            const float2 np = load_np(st, total, j, sl);
            sd += np.x;
            if (DIR) order += order_hit(np.x);
            apply_segment<B, LOBES>(E, np.x, load_mat(st, total, j, sl), np.y, kp, sc);
        }
        };
        if (ppw == 1u || (ppw <= 8u && st.over_levels != 0)) {
            // Few pairs per wave (the reference's own frames: one; ticks of several sources with uncapped walks: up to eight, of
            // which a fifth connect — and a connected path of uncapped walks has up to a few hundred segments, 40 us of ONE
            // lane's time at 160): the wave's 64 lanes evaluate a connected path together — lane i the factors of segment i
            // (64 segments per round), then every lane runs the same product over them in path order, the factors read across
            // with v_readlane — one connected pair of the wave after the other; the pair's own lane keeps the result and deposits.
            bool go = active && !hit && !sphere_blocked;
            if (go && st.over_levels && !(rec_fits(st, (int)Fm.y - 1, sf) && rec_fits(st, (int)Lm.y - 1, sl))) go = false;
            unsigned long long todo = __ballot(go);
            if (todo == 0ull) return;
            const float my_nd = (EXT && kp.dpos) ? conn_nd : sqrtf(l2) / kp.dist_divisor;
            while (todo != 0ull) {                                       // (wave-uniform)
                const int o = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const int kf = __builtin_amdgcn_readlane((int)Fm.y, o), kl = __builtin_amdgcn_readlane((int)Lm.y, o);
                const uint32_t usf = (uint32_t)__builtin_amdgcn_readlane((int)sf, o), usl = (uint32_t)__builtin_amdgcn_readlane((int)sl, o);
                const float c_nd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_nd), o));
                const uint32_t c_mat = (uint32_t)__builtin_amdgcn_readlane((int)Fm.x, o);
                const float c_prob = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(F.w), o));
                const int segs = kf + 1 + kl;
                float Et[Bands<B>::kMax];
#pragma unroll
                for (int b = 0; b < Bands<B>::kMax; ++b) Et[b] = 1.0f;
                float sdt = 0.0f;
                [[maybe_unused]] int ordt = 0;
                for (int base = 0; base < segs; base += 64) {
                    const int i = base + (int)lane;
                    float nd = 0.0f, prob = 1.0f;
                    uint32_t mat = kNoMat;
                    if (i < kf) {                                            // source-side segment F_i -> F_i+1
                        const float2 np = load_np(st, total, i, usf);
                        nd = np.x; prob = np.y; mat = load_mat(st, total, i, usf);
                    } else if (i == kf) {                                    // connection segment: F_k's material / prob
                        nd = c_nd; prob = c_prob; mat = c_mat;
                    } else if (i < segs) {                                   // listener-side segment B_j+1 -> B_j, j = kl - 1 .. 0
                        const int j = kl - 1 - (i - kf - 1);
                        const float2 np = load_np(st, total, j, usl);
                        nd = np.x; prob = np.y; mat = load_mat(st, total, j, usl);
                    }
                    // (DIR) the walk records among this round's segments that a hit made: every one but the connection segment
                    if (DIR) ordt += __popcll(__ballot(i < segs && i != kf && order_hit(nd) != 0));
                    SegFactors<B> f;
                    segment_factors<B, LOBES>(f, nd, mat, prob, kp, sc);
                    const int cnt = min(64, segs - base);
                    for (int q = 0; q < cnt; ++q) {                          // (wave-uniform: the product in path order, in every lane alike)
                        sdt += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nd), q));                 // ARTS.cpp:374
                        if (!__builtin_amdgcn_readlane((int)f.live, q)) continue;
                        const float geo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f.geo), q));
                        const float pw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f.pw), q));
#pragma unroll
                        for (int b = 0; b < Bands<B>::kMax; ++b) {
                            if (B == 0 && b >= NB) break;
                            float e = Et[b];
                            e *= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f.bsdf[b]), q));
                            e *= geo;
                            e *= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f.ex[b]), q));
                            e /= pw;
                            Et[b] = e;
                        }
                    }
                }
                if ((int)lane == o) {
#pragma unroll
                    for (int b = 0; b < Bands<B>::kMax; ++b) E[b] = Et[b];
                    sd = sdt;
                    if (DIR) order = ordt;
                }
            }
            if (!go) return;
            if (!DIR) ++my_deposits;
        } else {
        if (!active || hit || sphere_blocked) return;
        // depth = 0 only: a walk that outlived the record store has raised the overflow word — the frame is void and will
        // be traced again (FS_ERR_OVERFLOW); its pair must not be evaluated, the records it would read do not exist
        if (st.over_levels && !(rec_fits(st, (int)Fm.y - 1, sf) && rec_fits(st, (int)Lm.y - 1, sl))) return;
        if (!DIR) ++my_deposits;
        eval_alone();
        }
        DirLookup dl;
        if (DIR) {
            const Directivity& d = dir.tab ? dir.tab[lc / kp.pairs_per_source] : dir.one;
            // the source's order window: a path outside it deposits nothing and is not counted — after the shared visibility
            // query and the evaluation, which every lane of the wave went through alike
            if (order < d.min_order || order > d.max_order) return;
            ++my_deposits;
            // w_e: the ray the source's walk left by, else (it never left) the connection ray as computed above
            float wx = ux, wy = uy, wz = uz;
            if (d.table) {   // (a window alone: no table, factor 1 — the emission ray is not needed)
                const int ke = emission_step(st, total, sf, (int)Fm.y);
                if (ke >= 0) emission_ray(kp, lc, ke, wx, wy, wz);
            }
            dl = dir_lookup(d, wx, wy, wz);
        }
        float delay = sd / kp.sound_speed;                            // ARTS.cpp:419
        float x = (delay * 1000.f) / 1.0f;                            // FSAC.h:89, BinSizeMs = 1
        float fl = floorf(x);
        int bin = !(fl > 0.0f) ? 0 : (fl >= (float)(nb - 1) ? nb - 1 : (int)fl);
        const bool near = bin < W;
        if (!fixed_dst && near) {
            atomicMin(&s_lo, bin);
            atomicMax(&s_hi, bin);
        }
#pragma unroll
        for (int b = 0; b < Bands<B>::kMax; ++b) {
            if (B == 0 && b >= NB) break;
            float e = E[b];
            e = (e < kp.energy_clamp) ? e : kp.energy_clamp;          // FMath::Min ARTS.cpp:410
            e *= kp.energy_gain;                                      // ARTS.cpp:413
            e *= kp.norm;                                             // ARTS.cpp:164-170
            if (DIR) e *= dir_gain(dl, b);                            // the source's directivity, last
            if (fixed_dst)   // deterministic mode: integer sum of 2^-40 quanta — exact, so order- and shard-independent
                atomicAdd(&fixed_dst[b * nb + bin], (unsigned long long)__double2ll_rn((double)e * kFixedScale));
            else if (near)
                atomicAdd(&s_hist[b * W + bin], e);                   // ds_add_f32
            else
                atomicAdd(&far_dst[b * nb + bin], e);                 // beyond the LDS window: global_atomic_add_f32
        }
    };
    // LDS histogram -> one source's energy buffer (touched bin range only); clear = rearm it for the next source
    auto flush = [&](float* dst, bool clear) {
        __syncthreads();
        const int lo = s_lo, hi = s_hi;
        if (hi >= lo) {
            const int span = hi - lo + 1;
            for (int i = threadIdx.x; i < NB * span; i += kBlock) {
                int b = i / span, bin = lo + (i - b * span);
                float v = s_hist[b * W + bin];
                if (v != 0.0f) atomicAdd(&dst[b * nb + bin], v);      // global_atomic_add_f32
                if (clear) s_hist[b * W + bin] = 0.0f;
            }
        }
        if (clear) {
            __syncthreads();
            if (threadIdx.x == 0) { s_lo = nb; s_hi = -1; }
            __syncthreads();
        }
    };

    if (BATCH) {
        const uint32_t nps = kp.pairs_per_source, sources = n / nps;
        const uint32_t chunks = (nps + per_block - 1) / per_block;   // per source
        int cur = -1;
        for (uint32_t it = bid; it < chunks * sources; it += nblocks) {
            const uint32_t sid = it / chunks;
            if ((int)sid != cur) {
                if (cur >= 0 && !fixed_tab) flush(energy_tab[cur], true);
                cur = (int)sid;
            }
            chunk(sid * nps + (it - sid * chunks) * per_block, (sid + 1) * nps, fixed_tab ? fixed_tab[sid] : nullptr,
                  energy_tab[sid]);
        }
        if (cur >= 0 && !fixed_tab) flush(energy_tab[cur], false);
    } else {
        for (uint32_t base = bid * per_block; base < n; base += nblocks * per_block) chunk(base, n, fixed, energy);
    }
#ifdef FS_WAVE_TIMELINE
    tl[3] = __builtin_amdgcn_s_memrealtime();   // all chunks evaluated and deposited into LDS
#endif
    if (COUNT) add_fetch_counts(queue_head, 5, cnt_nv, cnt_nt);
    {   // work counters: summed per wave, then per workgroup in LDS — one global atomic per workgroup (thousands of
        // atomics on one address cost the kernel ~10 %)
        unsigned d = my_deposits, t = my_tested, g = my_segments;
        for (int o = 32; o > 0; o >>= 1) { d += __shfl_down(d, o); t += __shfl_down(t, o); g += __shfl_down(g, o); }
        if ((threadIdx.x & 63u) == 0u && d) atomicAdd(&s_dep, d);
        if ((threadIdx.x & 63u) == 0u && t) atomicAdd(&s_tst, t);
        if ((threadIdx.x & 63u) == 0u && g) atomicAdd(&s_sgs, g);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* counters = reinterpret_cast<unsigned long long*>(queue_head + kCounterWord);
        if (s_dep) atomicAdd(&counters[2], (unsigned long long)s_dep);
        if (s_tst) atomicAdd(&counters[1], (unsigned long long)s_tst);   // the pairs this workgroup's lanes tested
        if (s_sgs) atomicAdd(&counters[0], (unsigned long long)s_sgs);   // fs_stats.segments: observed (planned: counters[7], by the plan pass)
    }
    if (!BATCH) {
        const int lo = s_lo, hi = s_hi;
        if (hi >= lo) {
            const int span = hi - lo + 1;
            for (int i = threadIdx.x; i < NB * span; i += kBlock) {
                int b = i / span, bin = lo + (i - b * span);
                float v = s_hist[b * W + bin];
                if (v != 0.0f) atomicAdd(&energy[b * nb + bin], v);       // global_atomic_add_f32
            }
        }
    }
#ifdef FS_WAVE_TIMELINE
    if ((threadIdx.x & 63u) == 0u && g_conn_buf) {
        unsigned long long* o = g_conn_buf + 8ull * (bid * (kBlock / 64) + (threadIdx.x >> 6));
        o[0] = tl[0]; o[1] = tl[1]; o[2] = tl[2]; o[3] = tl[3]; o[4] = __builtin_amdgcn_s_memrealtime();
        o[5] = my_deposits; o[6] = 0; o[7] = 0;
    }
#endif
}

}  // namespace
}  // namespace fs
