// fs_connect_all.inc — the body of connect_all_kernel (FS_CONNECT_ALL_DIR 0) and of its directional form connect_all_dir_kernel
// (FS_CONNECT_ALL_DIR 1), included twice by fs_connect.hip.  The body is written out in each kernel rather than inlined from
// a shared device function: as an inlined function it changes the plain kernel's schedule (and its code is kept as it was).
// DIR: the source's directivity (fs_source_set_directivity) — w_e of (i, j) is the walk's emitting ray if F_0..F_i has left
// the source, else the direction of the connection F_i -> B_j; D_b(w_e) is the deposit's last factor.  The same entry applies
// the source's order window (fs_source_set_order_window): (i, j) whose hits among F1..Fi and B1..Bj lie outside it is dropped.
#if FS_CONNECT_ALL_DIR
template <int B>
__global__ __launch_bounds__(kBlock) void connect_all_dir_kernel(DeviceScene sc, KParams kp, SubpathState st,
                                                                 float* __restrict__ energy,
                                                                 unsigned long long* __restrict__ fixed,
                                                                 unsigned* queue_head, DirArgs dir) {
    constexpr bool DIR = true;
#else
template <int B>
__global__ __launch_bounds__(kBlock) void connect_all_kernel(DeviceScene sc, KParams kp, SubpathState st,
                                                             float* __restrict__ energy,
                                                             unsigned long long* __restrict__ fixed,
                                                             unsigned* queue_head) {
    constexpr bool DIR = false;
    [[maybe_unused]] const DirArgs dir{};   // (every use is under DIR)
#endif
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] stack | [B][hist_window] histogram
    int* s_stack = s_dyn;
    float* s_hist = reinterpret_cast<float*>(s_dyn + (size_t)sc.stack_rows * kBlock);
    const int nb = kp.num_bins, W = kp.hist_window, NB = band_count<B>(kp);
    int* s_share = reinterpret_cast<int*>(s_hist + (size_t)NB * W);   // work-sharing area of trav_any_shared
    __shared__ int s_lo, s_hi;
    for (int i = threadIdx.x; i < NB * W; i += kBlock) s_hist[i] = 0.0f;
    if (threadIdx.x == 0) { s_lo = nb; s_hi = -1; }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 1 + 2 * kPlanBuckets; i += kBlock) queue_head[i] = 0u;
    __syncthreads();

    const uint32_t n = kp.num_local;
    const uint32_t total = 2u * n;
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = threadIdx.x >> 6, waves = kBlock / 64;
    unsigned my_deposits = 0, my_tests = 0, my_segments = 0;
    for (uint32_t li = blockIdx.x * waves + wave; li < n; li += gridDim.x * waves) {
        const uint32_t sf = slot_of(st, li), sl = slot_of(st, n + li);
        const uint2 Fm = st.end_misc[sf];
        const uint2 Lm = st.end_misc[sl];
        const int kf = (int)Fm.y, kl = (int)Lm.y;
        if (lane == 0) my_segments += (unsigned)(kf + kl);   // fs_stats.segments: the steps the two walks took
        // depth = 0 only: a walk that outlived the record store (overflow word raised, the frame is traced again)
        if (st.over_levels && !(rec_fits(st, kf - 1, sf) && rec_fits(st, kl - 1, sl))) continue;
        [[maybe_unused]] int ke = -1;                  // DIR: the step the source's walk left by (wave-uniform: the wave's pair)
        [[maybe_unused]] float ex = 0.0f, ey = 0.0f, ez = 0.0f;
        if constexpr (DIR) {
            ke = emission_step(st, total, sf, kf);
            if (ke >= 0) emission_ray(kp, li, ke, ex, ey, ez);
        }
        const int combos = (kf + 1) * (kl + 1);
        for (int c0 = 0; c0 < combos; c0 += 64) {   // wave-uniform trip count: all lanes share the visibility queries
            const bool active = c0 + lane < combos;
            const int c = active ? c0 + lane : 0;
            if (active) ++my_tests;
            const int i = c / (kl + 1), j = c - i * (kl + 1);
            // node Fi (position, material, probability) and node Bj (position)
            float fx = kp.src[0], fy = kp.src[1], fz = kp.src[2];
            if (i > 0) { const float4 q = load_pos(st, total, i - 1, sf); fx = q.x; fy = q.y; fz = q.z; }
            float bx = kp.lis[0], by = kp.lis[1], bz = kp.lis[2];
            if (j > 0) { const float4 q = load_pos(st, total, j - 1, sl); bx = q.x; by = q.y; bz = q.z; }
            uint32_t fmat; float fprob;
            if (i < kf) { fmat = load_mat(st, total, i, sf); fprob = load_np(st, total, i, sf).y; }
            else { fmat = Fm.x; fprob = st.end_pos[sf].w; }
            fmat &= 0xFFFFu;   // a connection vertex scatters diffusely whatever lobe the walk took there later (row f4)
            float dx = bx - fx, dy = by - fy, dz = bz - fz;
            float l2 = dx * dx + dy * dy + dz * dz;
            float len = sqrtf(l2);
            float inv = 1.0f / len;
            float tmax = len - kp.connect_pullback;
            bool has_ray = active && (l2 > 1e-8f) && (tmax > 0.0f);
            Ray ray = make_ray(fx, fy, fz, dx * inv, dy * inv, dz * inv);
            bool sphere_blocked = false;   // the end points' collision spheres (SURVEY A.6-h): ConnectSubpaths ignores no actor
            if (has_ray && (kp.listener_radius > 0.0f || kp.source_radius > 0.0f)) {
                float ts;
                sphere_blocked = (kp.listener_radius > 0.0f && sphere_hit(ray, kp.lis, kp.listener_radius, tmax, ts)) ||
                                 (kp.source_radius > 0.0f && sphere_hit(ray, kp.src, kp.source_radius, tmax, ts));
                if (sphere_blocked) has_ray = false;
            }
            const bool hit = trav_any_shared(sc, has_ray, ray, tmax, &s_stack[threadIdx.x], s_share);
            if (!active || hit || sphere_blocked) continue;
            if constexpr (!DIR) ++my_deposits;
            float E[Bands<B>::kMax];
#pragma unroll
            for (int b = 0; b < Bands<B>::kMax; ++b) E[b] = 1.0f;
            float sd = 0.0f;
            [[maybe_unused]] int order = 0;   // DIR: the hits among F1..Fi and B1..Bj, counted as their records go by
            for (int a = 0; a < i; ++a) {                                 // F_a -> F_a+1
                const float2 np = load_np(st, total, a, sf);
                sd += np.x;
                if constexpr (DIR) order += order_hit(np.x);
                apply_segment<B>(E, np.x, load_mat(st, total, a, sf), np.y, kp, sc);
            }
            {                                                             // Fi -> Bj
                float nd = sqrtf(l2) / kp.dist_divisor;
                sd += nd;
                apply_segment<B>(E, nd, fmat, fprob, kp, sc);
            }
            for (int a = j - 1; a >= 0; --a) {                            // B_a+1 -> B_a
                const float2 np = load_np(st, total, a, sl);
                sd += np.x;
                if constexpr (DIR) order += order_hit(np.x);
                uint32_t bmat = load_mat(st, total, a, sl);
                if (a == j - 1) bmat &= 0xFFFFu;                          // Bj is the other connection vertex
                apply_segment<B>(E, np.x, bmat, np.y, kp, sc);
            }
            [[maybe_unused]] const Directivity* dsc = nullptr;
            if constexpr (DIR) {   // the order window: (i, j) outside it deposits nothing; strategy counts and densities below are everybody's
                dsc = dir.tab ? &dir.tab[li / kp.pairs_per_source] : &dir.one;
                if (order < dsc->min_order || order > dsc->max_order) continue;
                ++my_deposits;
            }
            const int t = i + j, D = kp.mis_depth;
            const int lo_t = t - D > 0 ? t - D : 0, hi_t = t < D ? t : D;
            float w = 1.0f / (float)(hi_t - lo_t + 1);
            if (kp.mis) w = mis_weight(kp, st, total, sf, sl, i, j);
            [[maybe_unused]] DirLookup dl;
            if constexpr (DIR) {
                const Directivity& d = *dsc;
                const bool left = ke >= 0 && ke < i;
                dl = dir_lookup(d, left ? ex : dx * inv, left ? ey : dy * inv, left ? ez : dz * inv);
            }
            float delay = sd / kp.sound_speed;
            float x = (delay * 1000.f) / 1.0f;
            float fl = floorf(x);
            int bin = !(fl > 0.0f) ? 0 : (fl >= (float)(nb - 1) ? nb - 1 : (int)fl);
            const bool near = bin < W;
            if (!fixed && near) {
                atomicMin(&s_lo, bin);
                atomicMax(&s_hi, bin);
            }
#pragma unroll
            for (int b = 0; b < Bands<B>::kMax; ++b) {
                if (B == 0 && b >= NB) break;
                float e = E[b];
                e = (e < kp.energy_clamp) ? e : kp.energy_clamp;
                e *= kp.energy_gain;
                e *= kp.norm;
                e *= w;
                if constexpr (DIR) e *= dir_gain(dl, b);
                if (fixed)
                    atomicAdd(&fixed[b * nb + bin], (unsigned long long)__double2ll_rn((double)e * kFixedScale));
                else if (near)
                    atomicAdd(&s_hist[b * W + bin], e);   // ds_add_f32.  (Summing the equal-bin deposits of a wave first —
                else                                      // ballot per distinct bin + butterfly per band — measured slower:
                    atomicAdd(&energy[b * nb + bin], e);  // 2.12 -> 2.47 ms at cfg3; a pair's paths rarely share a bin.)
            }
        }
    }
    {   // work counters: one atomic per wave
        unsigned long long* counters = reinterpret_cast<unsigned long long*>(queue_head + kCounterWord);
        unsigned d = my_deposits, t = my_tests;
        for (int o = 32; o > 0; o >>= 1) { d += __shfl_down(d, o); t += __shfl_down(t, o); }
        if (lane == 0) {
            if (my_segments) atomicAdd(&counters[0], (unsigned long long)my_segments);
            if (d) atomicAdd(&counters[2], (unsigned long long)d);
            if (t) atomicAdd(&counters[1], (unsigned long long)t);
        }
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    if (hi < lo) return;
    const int span = hi - lo + 1;
    for (int i = threadIdx.x; i < NB * span; i += kBlock) {
        int b = i / span, bin = lo + (i - b * span);
        float v = s_hist[b * W + bin];
        if (v != 0.0f) atomicAdd(&energy[b * nb + bin], v);
    }
}
