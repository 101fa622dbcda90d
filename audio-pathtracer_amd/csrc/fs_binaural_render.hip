// fs_binaural_render.hip — the binaural voices of all rows of one audio callback (fs_binaural_render_process_batch): per source a
// bank of voices as the reflection renderer's (fs_reflect_render.hip), each with one gain and, per ear, the head-related impulse
// response of the set direction nearest to the voice's direction folded into the voice's band FIR.  The reference has no slot for it.
//
// The rule is include/frequensee.h's, to the bit: the file is built with the library's -ffp-contract=off, every fp32 operation
// rounds on its own, in the order written.  The voice's block and the voice bank's two passes are fs_dev_render.hpp's, the one text
// the render kernels are built from; this file says what a binaural voice carries beyond a delay and band gains — a gain and an
// HRIR index — and folds the tap tables {c0[t], dc[t]} its render pass loads.
//
// Which slot continues, ends or starts is decided on the host (VoiceBankItem::op); four launches, whatever the number of rows — five
// with a mesh on the set (fs_hrtf_set_mesh), where a voice's HRIR is the blend of the three at the corners of the spherical
// triangle its direction falls in: the mode is the call's, chosen in launch_binaural_render, and the kernels of nearest mode keep
// their code:
//   locate  (with a mesh only) one wave per sounding slot, ending slots leave at once: the lanes stride over the triangles with
//           fs_internal.hpp's hrtf_mesh_scan — a lane's triangle is three 16-byte requests, a wave's 64 are 3 KiB in one piece —
//           a butterfly of hrtf_mesh_better leaves the best (mu, j) in every lane, and lane 0 writes {t1, b1[3]} for the plan pass.
//           No LDS, no atomics, one 16-byte store at an index the host's list gave.
//   plan    one thread per (row, slot): voice_bank_plan with the gain and the argmax of the entry's direction over the set's
//           directions (the lowest index among equals) as the aim, plus the slot's place in the folded tables.
//   fold    one workgroup per (sounding slot, ear): f0 = sum_b g0_b k_b and f1 = sum_b g1_b k_b and the two HRIRs h[q0][ear],
//           h[q1][ear] into LDS, then one thread per u of C_A[u] = sum_k h_A[k] f_A[u - k], k ascending, and {C0[u], C1[u] - C0[u]}
//           into the call's folded tables (with a mesh: h_A = (bA_0 h[v_0] + bA_1 h[v_1]) + bA_2 h[v_2] as LDS is filled, the loop
//           as it is).  Lanes of a wave read one h[k] (a broadcast) and neighbouring f[u - k]; where the lower
//           bound of k differs between lanes the h reads are neighbours too: no bank conflicts either way.  A slot whose band gains
//           and HRIR index did not change folds once: C1 has C0's bits.  With onsets on the set (fs_hrtf_set_onsets) h_A is the
//           HRIR delayed by the end's onset, of He = H + (int)omax + 1 taps (fs_internal.hpp's hrtf_delay_tap as LDS is filled, two
//           more instantiations — four in all —, the loop as it is, on He taps).
//   render  voice_bank_render, loading s_cd from the folded table of (slot, ear), with Tc = T + H - 1 taps (He in H's place with
//           onsets: the host's b.tc); ear ch reads channel
//           ch of the ring and of the block.
//   mix     one thread per sample, rows in list order (launch_callback_mix, fs_reverb.hip: the audio callbacks' one mix).
#include "fs_dev_render.hpp"

namespace fs {
namespace {

constexpr int kBrFoldThreads = 256;

struct BinauralVoices {
    struct Aim { float w; int q; };   // the gain, the HRIR index
    static __device__ __forceinline__ Aim read(const fs_binaural_voice& v, const float* __restrict__ dirs, int n_dirs) {
        int q = 0;
        float best = (v.direction[0] * dirs[0] + v.direction[1] * dirs[1]) + v.direction[2] * dirs[2];
        for (int j = 1; j < n_dirs; ++j) {
            const float* __restrict__ p = dirs + 3 * (size_t)j;
            const float dot = (v.direction[0] * p[0] + v.direction[1] * p[1]) + v.direction[2] * p[2];
            if (dot > best) { best = dot; q = j; }   // (an equal later one does not replace it: the lowest index)
        }
        return {v.gain, q};
    }
    static __device__ __forceinline__ Aim fade_out(const BinauralRenderSlot& st) { return {0.0f, st.q0}; }   // (the HRIR stays)
    static __device__ __forceinline__ void from_silence(BinauralRenderSlot& st, const Aim& aim) {
        st.w0 = 0.0f;
        st.q0 = aim.q;
    }
    static __device__ __forceinline__ void plan(BinauralRenderPlan& pl, const BinauralRenderSlot& st, const Aim& aim, const BinauralRenderItem& it,
                                                int slot) {
        pl.w0 = st.w0;
        pl.dw = aim.w - st.w0;
        pl.q0 = st.q0;
        pl.q1 = aim.q;
        pl.index = it.first;   // sounding slots below this one
        for (int j = 0; j < slot; ++j) pl.index += it.op[j] != kVoiceIdle;
        pl.pad = 0;
    }
    static __device__ __forceinline__ void keep(BinauralRenderSlot& st, const Aim& aim) {
        st.w0 = aim.w;
        st.q0 = aim.q;
    }
};

// ... and with a mesh: the triangle t and the weights b[3] in q's place.  What the locate pass found for the thread's (row, slot)
// is read at the thread's own index — voice_bank_plan's: one thread per (row, slot).
struct BinauralMeshVoices {
    struct Aim { float w; int t; float b[3]; };
    static __device__ __forceinline__ Aim read(const fs_binaural_voice& v, const float4* __restrict__ located) {
        const float4 at = located[blockIdx.x * blockDim.x + threadIdx.x];
        return {v.gain, (int)__float_as_uint(at.x), {at.y, at.z, at.w}};
    }
    static __device__ __forceinline__ Aim fade_out(const BinauralRenderSlot& st) {   // (the triangle and the weights stay)
        return {0.0f, st.q0, {__int_as_float(st.pad[0]), __int_as_float(st.pad[1]), __int_as_float(st.pad[2])}};
    }
    static __device__ __forceinline__ void from_silence(BinauralRenderSlot& st, const Aim& aim) {
        st.w0 = 0.0f;
        keep_aim(st, aim);
    }
    static __device__ __forceinline__ void plan(BinauralMeshPlan& pl, const BinauralRenderSlot& st, const Aim& aim, const BinauralRenderItem& it,
                                                int slot) {
        BinauralVoices::plan(pl, st, {aim.w, 0}, it, slot);
        pl.q0 = 0;
        pl.t0 = st.q0;
        pl.t1 = aim.t;
        for (int i = 0; i < 3; ++i) { pl.b0[i] = __int_as_float(st.pad[i]); pl.b1[i] = aim.b[i]; }
    }
    static __device__ __forceinline__ void keep(BinauralRenderSlot& st, const Aim& aim) {
        st.w0 = aim.w;
        keep_aim(st, aim);
    }
    static __device__ __forceinline__ void keep_aim(BinauralRenderSlot& st, const Aim& aim) {
        st.q0 = aim.t;
        for (int i = 0; i < 3; ++i) st.pad[i] = __float_as_int(aim.b[i]);
    }
};

// The two HRIRs a slot's fold runs on, per mode: whether they are one (so that, the band gains being equal too, one fold serves
// both ends — compared by bits, so that -0 is not +0), and tap k of end A for the LDS fill.
struct FoldNearest {
    int q0, q1;
    __device__ __forceinline__ FoldNearest(const BinauralRenderPlan* __restrict__ plp, const float4* __restrict__, int) : q0(plp->q0), q1(plp->q1) {}
    __device__ __forceinline__ bool same() const { return q0 == q1; }
    __device__ __forceinline__ float2 tap(const float* __restrict__ hrir, int ear, int h_taps, int k) const {
        return make_float2(hrir[((size_t)q0 * 2 + (size_t)ear) * (size_t)h_taps + k], hrir[((size_t)q1 * 2 + (size_t)ear) * (size_t)h_taps + k]);
    }
};
struct FoldMesh {
    int t[2], v[2][3];
    float b[2][3];
    __device__ __forceinline__ FoldMesh(const BinauralMeshPlan* __restrict__ plp, const float4* __restrict__ mesh, int) {
        t[0] = plp->t0; t[1] = plp->t1;
        for (int i = 0; i < 3; ++i) {
            b[0][i] = plp->b0[i]; b[1][i] = plp->b1[i];
            v[0][i] = (int)__float_as_uint(mesh[(size_t)t[0] * 3 + i].w);
            v[1][i] = (int)__float_as_uint(mesh[(size_t)t[1] * 3 + i].w);
        }
    }
    __device__ __forceinline__ bool same() const {
        bool s = t[0] == t[1];
        for (int i = 0; i < 3; ++i) s = s && __float_as_uint(b[0][i]) == __float_as_uint(b[1][i]);
        return s;
    }
    __device__ __forceinline__ float end(const float* __restrict__ hrir, int ear, int h_taps, int k, int A) const {
        const float h0 = hrir[((size_t)v[A][0] * 2 + (size_t)ear) * (size_t)h_taps + k];
        const float h1 = hrir[((size_t)v[A][1] * 2 + (size_t)ear) * (size_t)h_taps + k];
        const float h2 = hrir[((size_t)v[A][2] * 2 + (size_t)ear) * (size_t)h_taps + k];
        return (b[A][0] * h0 + b[A][1] * h1) + b[A][2] * h2;
    }
    __device__ __forceinline__ float2 tap(const float* __restrict__ hrir, int ear, int h_taps, int k) const {
        return make_float2(end(hrir, ear, h_taps, k, 0), end(hrir, ear, h_taps, k, 1));
    }
};

// ... and with onsets on the set (fs_hrtf_set_onsets): the set's HRIRs are read as aligned, of `set_taps` taps, and tap k of end A
// is that of the HRIR delayed by tauA — the onset of qA, or with a mesh the blend of the three corners' onsets, clamped to omax —
// for k up to h_taps = He.  The aligned HRIR is evaluated at the two indices a tap reads (hrtf_delay_tap), 0.0f outside the set's
// taps: no second LDS array and no further barrier; neighbouring k read neighbouring addresses, so the requests stay coalesced.
// Equal q, or equal (t, b) bits, give equal tau bits: same() is the mode's own.
struct FoldNearestOnsets : FoldNearest {
    HrtfDelay d[2];
    int set_taps;
    __device__ __forceinline__ FoldNearestOnsets(const BinauralRenderPlan* __restrict__ plp, const float4* __restrict__ mesh, int ear,
                                                 const float* __restrict__ onsets, float omax, int set_taps_)
        : FoldNearest(plp, mesh, ear), set_taps(set_taps_) {
        const int q[2] = {q0, q1};
        for (int A = 0; A < 2; ++A) {
            float tau = onsets[(size_t)q[A] * 2 + (size_t)ear];
            if (tau > omax) tau = omax;
            d[A] = hrtf_delay_of(tau);
        }
    }
    __device__ __forceinline__ float end(const float* __restrict__ hrir, int ear, int k, int A) const {
        const float* __restrict__ h = hrir + ((size_t)(A ? q1 : q0) * 2 + (size_t)ear) * (size_t)set_taps;
        const int H = set_taps;
        return hrtf_delay_tap(d[A], k, [=](int j) { return j >= 0 && j < H ? h[j] : 0.0f; });
    }
    __device__ __forceinline__ float2 tap(const float* __restrict__ hrir, int ear, int, int k) const {
        return make_float2(end(hrir, ear, k, 0), end(hrir, ear, k, 1));
    }
};
struct FoldMeshOnsets : FoldMesh {
    HrtfDelay d[2];
    int set_taps;
    __device__ __forceinline__ FoldMeshOnsets(const BinauralMeshPlan* __restrict__ plp, const float4* __restrict__ mesh, int ear,
                                              const float* __restrict__ onsets, float omax, int set_taps_)
        : FoldMesh(plp, mesh, ear), set_taps(set_taps_) {
        for (int A = 0; A < 2; ++A) {
            const float o0 = onsets[(size_t)v[A][0] * 2 + (size_t)ear], o1 = onsets[(size_t)v[A][1] * 2 + (size_t)ear];
            const float o2 = onsets[(size_t)v[A][2] * 2 + (size_t)ear];
            float tau = (b[A][0] * o0 + b[A][1] * o1) + b[A][2] * o2;
            if (tau > omax) tau = omax;   // (the weights sum to 1 only within 2 ulp: the last tap stays inside He)
            d[A] = hrtf_delay_of(tau);
        }
    }
    __device__ __forceinline__ float2 tap(const float* __restrict__ hrir, int ear, int, int k) const {
        const int H = set_taps;
        const FoldMesh& blend = *this;
        float2 out;
        out.x = hrtf_delay_tap(d[0], k, [&](int j) { return j >= 0 && j < H ? blend.end(hrir, ear, H, j, 0) : 0.0f; });
        out.y = hrtf_delay_tap(d[1], k, [&](int j) { return j >= 0 && j < H ? blend.end(hrir, ear, H, j, 1) : 0.0f; });
        return out;
    }
};

__global__ void binaural_render_plan_kernel(const BinauralRenderItem* __restrict__ items, const fs_binaural_voice* __restrict__ voices,
                                            const float* __restrict__ dirs, int n_dirs, BinauralRenderPlan* __restrict__ plans,
                                            unsigned* __restrict__ n0_out, int count, int stride, int frame, int bands, float fs_f) {
    voice_bank_plan<BinauralVoices>(items, voices, plans, n0_out, count, stride, frame, bands, fs_f, dirs, n_dirs);
}

constexpr int kBrLocateThreads = 256;   // four waves, a sounding slot each

__global__ __launch_bounds__(kBrLocateThreads) void binaural_render_locate_kernel(const BinauralRenderItem* __restrict__ items,
                                                                                   const uint16_t* __restrict__ sounding,
                                                                                   const fs_binaural_voice* __restrict__ voices,
                                                                                   const float4* __restrict__ mesh, int n_tris,
                                                                                   float4* __restrict__ located, int n_sounding, int stride) {
    const int wave = (int)(blockIdx.x * kBrLocateThreads + threadIdx.x) / 64, lane = threadIdx.x & 63;
    if (wave >= n_sounding) return;   // (uniform over the wave, as every branch before the butterfly)
    const int which = sounding[wave];
    const int r = which / kVoiceSlots;
    const int op = items[r].op[which % kVoiceSlots];
    if (op == kVoiceEnd || op == kVoiceIdle) return;   // no entry: the slot keeps its triangle (idle: never listed)
    const fs_binaural_voice* __restrict__ v = voices + (size_t)r * (size_t)stride + (size_t)(op >= kVoiceStart ? op - kVoiceStart : op - kVoiceContinue);
    const float d[3] = {v->direction[0], v->direction[1], v->direction[2]};
    const HrtfMeshRowsDevice rows = {mesh};
    HrtfMeshBest best = hrtf_mesh_scan(rows, n_tris, d, lane, 64);
    for (int off = 32; off > 0; off >>= 1) {
        const HrtfMeshBest other = {__shfl_xor(best.mu, off), __shfl_xor(best.j, off)};
        if (hrtf_mesh_better(other, best)) best = other;
    }
    if (lane != 0) return;
    float b[3];
    hrtf_mesh_weights(rows, best.j, d, b);
    located[which] = make_float4(__uint_as_float((unsigned)best.j), b[0], b[1], b[2]);
}

__global__ void binaural_render_mesh_plan_kernel(const BinauralRenderItem* __restrict__ items, const fs_binaural_voice* __restrict__ voices,
                                                 const float4* __restrict__ located, BinauralMeshPlan* __restrict__ plans,
                                                 unsigned* __restrict__ n0_out, int count, int stride, int frame, int bands, float fs_f) {
    voice_bank_plan<BinauralMeshVoices>(items, voices, plans, n0_out, count, stride, frame, bands, fs_f, located);
}

// (h_taps: the taps of the HRIRs the fold runs on — H, with onsets He; Extra: what the Ends of a mode with onsets read beyond the
// plan and the mesh — the onsets, omax and the set's own H —, nothing in the two modes without)
template <typename Ends, typename Plan, typename... Extra>
__global__ __launch_bounds__(kBrFoldThreads) void binaural_render_fold_kernel(const BinauralRenderItem* __restrict__ items,
                                                                               const uint16_t* __restrict__ sounding,
                                                                               const Plan* __restrict__ plans,
                                                                               const float* __restrict__ hrir, const float4* __restrict__ mesh,
                                                                               float2* __restrict__ folded, int taps, int h_taps, int bands,
                                                                               Extra... extra) {
    __shared__ float s_f[2][kRenderMaxTaps];        // f0, f1
    __shared__ float s_h[2][FS_MAX_HRTF_TAPS];      // h_0, h_1: h[q0][ear], h[q1][ear], or the blends
    const int which = sounding[blockIdx.x];
    const int ear = blockIdx.y;
    const int tid = threadIdx.x;
    const Plan* __restrict__ plp = plans + which;   // (which = row * kVoiceSlots + slot: the plans' own index)
    const float* __restrict__ table = items[which / kVoiceSlots].table;
    const Ends ends(plp, mesh, ear, extra...);
    // (uniform over the workgroup) nothing ramps: one fold serves both ends — compared by bits, so that -0 is not +0
    bool same = ends.same();
    for (int b = 0; b < bands; ++b) same = same && __float_as_uint(plp->g0[b]) == __float_as_uint(plp->g1[b]);
    for (int t = tid; t < taps; t += kBrFoldThreads) {   // render_build_taps' sums
        float c0 = 0.0f, c1 = 0.0f;
        for (int b = 0; b < bands; ++b) {
            const float k = table[(size_t)b * (size_t)taps + t];
            c0 = c0 + plp->g0[b] * k;
            c1 = c1 + plp->g1[b] * k;
        }
        s_f[0][t] = c0;
        s_f[1][t] = c1;
    }
    for (int k = tid; k < h_taps; k += kBrFoldThreads) {
        const float2 h = ends.tap(hrir, ear, h_taps, k);
        s_h[0][k] = h.x;
        s_h[1][k] = h.y;
    }
    __syncthreads();
    const int tc = taps + h_taps - 1;
    float2* __restrict__ dst = folded + ((size_t)plp->index * 2 + (size_t)ear) * (size_t)tc;
    for (int u = tid; u < tc; u += kBrFoldThreads) {
        const int k_lo = max(0, u - taps + 1), k_hi = min(h_taps - 1, u);
        float c0 = 0.0f, c1 = 0.0f;
        if (same) {
            for (int k = k_lo; k <= k_hi; ++k) c0 = c0 + s_h[0][k] * s_f[0][u - k];
            c1 = c0;
        } else {
            for (int k = k_lo; k <= k_hi; ++k) {
                c0 = c0 + s_h[0][k] * s_f[0][u - k];
                c1 = c1 + s_h[1][k] * s_f[1][u - k];
            }
        }
        dst[u] = make_float2(c0, c1 - c0);
    }
}

template <typename Plan>   // (BinauralRenderPlan, or with a mesh the wider BinauralMeshPlan: the stride of `plans`)
__global__ __launch_bounds__(kRenderTile) void binaural_render_kernel(const BinauralRenderItem* __restrict__ items,
                                                                       const Plan* __restrict__ plans,
                                                                       const float2* __restrict__ folded, const unsigned* __restrict__ n0_all,
                                                                       const float* __restrict__ in_all, float* __restrict__ out_all, int frame,
                                                                       int tc) {
    voice_bank_render(
        items, plans, n0_all, in_all, out_all, frame, tc,
        [=](RenderTaps& s_cd, const float*, const Plan* __restrict__ plp, int ch, int tid) {   // (ch: the ear)
            render_load_taps(s_cd, folded + ((size_t)plp->index * 2 + (size_t)ch) * (size_t)tc, tc, tid);
        },
        [](const Plan* __restrict__ plp, int) { return make_float2(plp->w0, plp->dw); });
}

}  // namespace

template <typename Ends, typename EndsOnsets, typename Plan>
static void launch_fold_render(const BinauralRenderBatch& b, const Plan* plans, hipStream_t s) {
    if (b.n_sounding > 0 && !b.onsets)   // (a callback of silent rows folds nothing)
        hipLaunchKernelGGL((binaural_render_fold_kernel<Ends, Plan>), dim3(b.n_sounding, 2), dim3(kBrFoldThreads), 0, s, b.items, b.sounding,
                           plans, b.hrir, b.mesh, b.folded, b.taps, b.h_taps, b.bands);
    else if (b.n_sounding > 0)
        hipLaunchKernelGGL((binaural_render_fold_kernel<EndsOnsets, Plan, const float*, float, int>), dim3(b.n_sounding, 2),
                           dim3(kBrFoldThreads), 0, s, b.items, b.sounding, plans, b.hrir, b.mesh, b.folded, b.taps, b.h_eff, b.bands,
                           b.onsets, b.omax, b.h_taps);
    const int tiles = (b.frame + kRenderTile - 1) / kRenderTile;
    hipLaunchKernelGGL(binaural_render_kernel<Plan>, dim3(tiles, 2, b.count), dim3(kRenderTile), 0, s, b.items, plans, b.folded, b.n0, b.in,
                       b.out, b.frame, b.tc);
}

void launch_binaural_render(const BinauralRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    if (b.mesh) {
        if (b.n_sounding > 0)
            hipLaunchKernelGGL(binaural_render_locate_kernel, dim3((b.n_sounding * 64 + kBrLocateThreads - 1) / kBrLocateThreads),
                               dim3(kBrLocateThreads), 0, s, b.items, b.sounding, b.voices, b.mesh, b.n_tris, b.located, b.n_sounding, b.stride);
        hipLaunchKernelGGL(binaural_render_mesh_plan_kernel, dim3((b.count * kVoiceSlots + tb - 1) / tb), dim3(tb), 0, s, b.items, b.voices,
                           b.located, b.mesh_plans, b.n0, b.count, b.stride, b.frame, b.bands, b.fs);
        launch_fold_render<FoldMesh, FoldMeshOnsets>(b, (const BinauralMeshPlan*)b.mesh_plans, s);
    } else {
        hipLaunchKernelGGL(binaural_render_plan_kernel, dim3((b.count * kVoiceSlots + tb - 1) / tb), dim3(tb), 0, s, b.items, b.voices, b.dirs,
                           b.n_dirs, b.plans, b.n0, b.count, b.stride, b.frame, b.bands, b.fs);
        launch_fold_render<FoldNearest, FoldNearestOnsets>(b, (const BinauralRenderPlan*)b.plans, s);
    }
    if (b.mix) launch_callback_mix(b.out, b.count, 2 * b.frame, b.mix, s);
}

}  // namespace fs
