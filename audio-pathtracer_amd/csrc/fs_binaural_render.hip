// fs_binaural_render.hip — the binaural voices of all rows of one audio callback (fs_binaural_render_process_batch): the voice bank
// of fs_reflect_render.hip with the per-channel gain pair replaced by one gain and, per ear, the head-related impulse response of
// the set direction nearest to the voice's direction folded into the voice's band FIR.  The reference has no slot for it.
//
// The rule is include/frequensee.h's, to the bit: the file is built with the library's -ffp-contract=off, every fp32 operation
// below rounds on its own, in the order written.  The voice's block — read window, tap loop, store — is fs_dev_render.hpp's, the
// one text the render kernels are built from; what differs is where the tap table {c0[t], dc[t]} comes from.
//
// Which slot continues, ends or starts is decided on the host (BinauralRenderItem::op); four launches, whatever the number of rows:
//   plan    one thread per (row, slot): the reflection renderer's plan pass with one gain for two, plus the argmax of the entry's
//           direction over the set's directions (the lowest index among equals) and the slot's place in the folded tables.
//   fold    one workgroup per (sounding slot, ear): f0 = sum_b g0_b k_b and f1 = sum_b g1_b k_b and the two HRIRs h[q0][ear],
//           h[q1][ear] into LDS, then one thread per u of C_A[u] = sum_k h_A[k] f_A[u - k], k ascending, and {C0[u], C1[u] - C0[u]}
//           into the call's folded tables.  Lanes of a wave read one h[k] (a broadcast) and neighbouring f[u - k]; where the lower
//           bound of k differs between lanes the h reads are neighbours too: no bank conflicts either way.  A slot whose band gains
//           and HRIR index did not change folds once: C1 has C0's bits.
//   render  the reflection kernel's loop, loading s_cd from the folded table of (slot, ear) instead of building it, with
//           Tc = T + H - 1 taps; ear ch reads channel ch of the ring and of the block.
//   mix     one thread per sample, rows in list order (launch_callback_mix, fs_reverb.hip: the audio callbacks' one mix).
#include "fs_dev_render.hpp"

namespace fs {
namespace {

constexpr int kBrSlots = FS_MAX_REFLECTION_VOICES;
constexpr int kBrFoldThreads = 256;

__global__ void binaural_render_plan_kernel(const BinauralRenderItem* __restrict__ items, const fs_binaural_voice* __restrict__ voices,
                                            const float* __restrict__ dirs, int n_dirs, BinauralRenderPlan* __restrict__ plans,
                                            unsigned* __restrict__ n0_out, int count, int stride, int frame, int bands, float fs_f) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = id / kBrSlots, slot = id % kBrSlots;
    if (r >= count) return;
    const BinauralRenderItem& it = items[r];
    if (slot == 0) {
        const unsigned n0 = it.state->n0;
        n0_out[r] = n0;
        it.state->n0 = n0 + (unsigned)frame;
    }
    if (slot >= it.slots) return;
    const int op = it.op[slot];
    if (op == kReflectIdle) return;
    int index = it.first;   // sounding slots below this one
    for (int j = 0; j < slot; ++j) index += it.op[j] != kReflectIdle;
    BinauralRenderSlot st = it.state->slot[slot];
    BinauralRenderPlan pl;
    float d1, g1[FS_MAX_BANDS], w1;
    int q1;
    if (op == kReflectEnd) {   // the delay freezes, the gains and the HRIR stay, the gain goes to 0
        d1 = st.d0;
        for (int b = 0; b < FS_MAX_BANDS; ++b) g1[b] = st.g0[b];
        w1 = 0.0f;
        q1 = st.q0;
    } else {
        const bool start = op >= kReflectStart;
        const fs_binaural_voice v = voices[(size_t)r * (size_t)stride + (size_t)(start ? op - kReflectStart : op - kReflectContinue)];
        d1 = v.delay * fs_f;
        for (int b = 0; b < FS_MAX_BANDS; ++b) g1[b] = v.band_gain[b];
        w1 = v.gain;
        q1 = 0;
        float best = (v.direction[0] * dirs[0] + v.direction[1] * dirs[1]) + v.direction[2] * dirs[2];
        for (int j = 1; j < n_dirs; ++j) {
            const float* __restrict__ p = dirs + 3 * (size_t)j;
            const float dot = (v.direction[0] * p[0] + v.direction[1] * p[1]) + v.direction[2] * p[2];
            if (dot > best) { best = dot; q1 = j; }   // (an equal later one does not replace it: the lowest index)
        }
        if (start) {   // from its target, out of silence
            st.d0 = d1;
            for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = g1[b];
            st.w0 = 0.0f;
            st.q0 = q1;
        }
        st.key = v.key;
    }
    const float e = render_slew(d1 - st.d0, frame);
    pl.d0 = st.d0;
    pl.e = e;
    for (int b = 0; b < FS_MAX_BANDS; ++b) { pl.g0[b] = st.g0[b]; pl.g1[b] = g1[b]; }
    pl.w0 = st.w0;
    pl.dw = w1 - st.w0;
    pl.q0 = st.q0;
    pl.q1 = q1;
    pl.index = index;
    pl.pad = 0;
    plans[(size_t)r * kBrSlots + slot] = pl;
    if (op == kReflectEnd) {
        st = BinauralRenderSlot{};   // free
    } else {
        st.held = 1;
        st.d0 = pl.d0 + e;   // what the last output sample used: a == 1 there
        for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = b < bands ? g1[b] : 0.0f;
        st.w0 = w1;
        st.q0 = q1;
    }
    it.state->slot[slot] = st;
}

__global__ __launch_bounds__(kBrFoldThreads) void binaural_render_fold_kernel(const BinauralRenderItem* __restrict__ items,
                                                                               const uint16_t* __restrict__ sounding,
                                                                               const BinauralRenderPlan* __restrict__ plans,
                                                                               const float* __restrict__ hrir, float2* __restrict__ folded,
                                                                               int taps, int h_taps, int bands) {
    __shared__ float s_f[2][kRenderMaxTaps];        // f0, f1
    __shared__ float s_h[2][FS_MAX_HRTF_TAPS];      // h[q0][ear], h[q1][ear]
    const int which = sounding[blockIdx.x];
    const int ear = blockIdx.y;
    const int tid = threadIdx.x;
    const BinauralRenderPlan* __restrict__ plp = plans + which;   // (which = row * kBrSlots + slot: the plans' own index)
    const float* __restrict__ table = items[which / kBrSlots].table;
    const int q0 = plp->q0, q1 = plp->q1;
    // (uniform over the workgroup) nothing ramps: one fold serves both ends — compared by bits, so that -0 is not +0
    bool same = q0 == q1;
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
        s_h[0][k] = hrir[((size_t)q0 * 2 + (size_t)ear) * (size_t)h_taps + k];
        s_h[1][k] = hrir[((size_t)q1 * 2 + (size_t)ear) * (size_t)h_taps + k];
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

__global__ __launch_bounds__(kRenderTile) void binaural_render_kernel(const BinauralRenderItem* __restrict__ items,
                                                                       const BinauralRenderPlan* __restrict__ plans,
                                                                       const float2* __restrict__ folded, const unsigned* __restrict__ n0_all,
                                                                       const float* __restrict__ in_all, float* __restrict__ out_all, int frame,
                                                                       int tc) {
    __shared__ RenderTaps s_cd;      // of the slot in hand
    __shared__ RenderWindow s_win;   // likewise: every slot has a delay of its own
    const int r = blockIdx.z;
    struct { float* ring; unsigned mask; int slots; } it = {items[r].ring, items[r].mask, items[r].slots};
    const int8_t* __restrict__ ops = items[r].op;
    const unsigned n0 = n0_all[r];
    const int ch = blockIdx.y;   // the ear
    const int s_a = blockIdx.x * kRenderTile;
    const int s_b = min(s_a + kRenderTile, frame) - 1;
    const int tid = threadIdx.x;
    const int s = s_a + tid;
    const bool live = s < frame;
    const float* __restrict__ in = in_all + (size_t)r * 2 * (size_t)frame;
    float* __restrict__ ring = it.ring + (size_t)ch * ((size_t)it.mask + 1);
    const float frame_f = (float)frame;
    float out = 0.0f;

    for (int slot = 0; slot < it.slots; ++slot) {   // (uniform over the workgroup: the row's)
        if (ops[slot] == kReflectIdle) continue;
        const BinauralRenderPlan* __restrict__ plp = plans + (size_t)r * kBrSlots + slot;
        struct { float d0, e, w0, dw; int index; } pl = {plp->d0, plp->e, plp->w0, plp->dw, plp->index};

        render_load_taps(s_cd, folded + ((size_t)pl.index * 2 + (size_t)ch) * (size_t)tc, tc, tid);
        const int i_hi = render_stage_window(s_win, ring, it.mask, in, ch, n0, pl.d0, pl.e, s_a, s_b, frame, frame_f, tc, tid);
        __syncthreads();

        if (live) {
            float a;
            const float y = render_sample(s_cd, s_win, pl.d0, pl.e, s, s_a, i_hi, frame_f, tc, &a);
            const float w = pl.w0 + a * pl.dw;
            out = out + w * y;
        }
        __syncthreads();   // the next slot rebuilds the LDS
    }
    if (!live) return;
    render_store(out_all, ring, it.mask, in, r, ch, n0, s, frame, out);
}

}  // namespace

void launch_binaural_render(const BinauralRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(binaural_render_plan_kernel, dim3((b.count * kBrSlots + tb - 1) / tb), dim3(tb), 0, s, b.items, b.voices, b.dirs,
                       b.n_dirs, b.plans, b.n0, b.count, b.stride, b.frame, b.bands, b.fs);
    if (b.n_sounding > 0)   // (a callback of silent rows folds nothing)
        hipLaunchKernelGGL(binaural_render_fold_kernel, dim3(b.n_sounding, 2), dim3(kBrFoldThreads), 0, s, b.items, b.sounding, b.plans,
                           b.hrir, b.folded, b.taps, b.h_taps, b.bands);
    const int tiles = (b.frame + kRenderTile - 1) / kRenderTile;
    hipLaunchKernelGGL(binaural_render_kernel, dim3(tiles, 2, b.count), dim3(kRenderTile), 0, s, b.items, b.plans, b.folded, b.n0, b.in,
                       b.out, b.frame, b.tc);
    if (b.mix) launch_callback_mix(b.out, b.count, b.frame, b.mix, s);
}

}  // namespace fs
