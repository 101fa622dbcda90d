// fs_reflect_render.hip — the early reflections of all rows of one audio callback (fs_reflection_render_process_batch): per source
// a bank of voices, each one the direct renderer's block (fs_direct_render.hip: a time-varying fractional delay and a linear-phase
// FIR whose taps are sum_b gain_b * k_b) reading the source's one history ring, weighted by a ramping per-channel gain and summed
// in ascending slot order.  The reference has no slot for it.
//
// The rule is include/frequensee.h's, to the bit: the file is built with the library's -ffp-contract=off, every fp32 operation
// below rounds on its own, in the order written.  The voice's block — tap table, read window, tap loop, store — is fs_dev_render.hpp's,
// the one text both render kernels are built from.
//
// Which slot continues, ends or starts is decided on the host (ReflectRenderItem::op); three launches, whatever the number of rows:
//   plan    one thread per (row, slot): reads the slot's device-resident state and the entry the host matched it with, fixes what
//           this callback ramps from and by how much in the slot's plan record, and writes the state the callback leaves behind;
//           the thread of slot 0 also moves the row's sample counter on.
//   render  a grid of (frame / 256 output tiles) x 2 channels x rows.  A workgroup loops over its row's sounding slots in ascending
//           order — the trip count and every branch around a barrier depend on the row only — and per slot builds the taps
//           {c0[t], dc[t]} and the tile's read window in LDS (the window is per slot: every slot has a delay of its own), runs
//           the four-accumulator tap loop of one output sample per thread and adds w * y to a register.  A thread past the frame's
//           end keeps building tables and windows and skips only the tap loop and the stores: nobody leaves before the last
//           barrier.  After the last slot the thread stores its output and appends its input sample to the ring: a callback reads
//           ring positions [n0 - D - T, n0) and writes [n0, n0 + F), disjoint modulo the ring because it holds D + T + 1 + F or more.
//   mix     one thread per sample, rows in list order (launch_callback_mix, fs_reverb.hip: the three callbacks' one mix).
#include "fs_dev_render.hpp"

namespace fs {
namespace {

constexpr int kRrSlots = FS_MAX_REFLECTION_VOICES;

__global__ void reflect_render_plan_kernel(const ReflectRenderItem* __restrict__ items, const fs_reflection_voice* __restrict__ voices,
                                           ReflectRenderPlan* __restrict__ plans, unsigned* __restrict__ n0_out, int count, int stride,
                                           int frame, int bands, float fs_f) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = id / kRrSlots, slot = id % kRrSlots;
    if (r >= count) return;
    const ReflectRenderItem& it = items[r];
    if (slot == 0) {
        const unsigned n0 = it.state->n0;
        n0_out[r] = n0;
        it.state->n0 = n0 + (unsigned)frame;
    }
    if (slot >= it.slots) return;
    const int op = it.op[slot];
    if (op == kReflectIdle) return;
    ReflectRenderSlot st = it.state->slot[slot];
    ReflectRenderPlan pl;
    float d1, g1[FS_MAX_BANDS], w1[2];
    if (op == kReflectEnd) {   // the delay freezes, the gains stay, the channel gains go to 0
        d1 = st.d0;
        for (int b = 0; b < FS_MAX_BANDS; ++b) g1[b] = st.g0[b];
        w1[0] = w1[1] = 0.0f;
    } else {
        const bool start = op >= kReflectStart;
        const fs_reflection_voice v = voices[(size_t)r * (size_t)stride + (size_t)(start ? op - kReflectStart : op - kReflectContinue)];
        d1 = v.delay * fs_f;
        for (int b = 0; b < FS_MAX_BANDS; ++b) g1[b] = v.band_gain[b];
        w1[0] = v.channel_gain[0];
        w1[1] = v.channel_gain[1];
        if (start) {   // from its target, out of silence
            st.d0 = d1;
            for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = g1[b];
            st.w0[0] = st.w0[1] = 0.0f;
        }
        st.key = v.key;
    }
    const float e = render_slew(d1 - st.d0, frame);
    pl.d0 = st.d0;
    pl.e = e;
    for (int b = 0; b < FS_MAX_BANDS; ++b) { pl.g0[b] = st.g0[b]; pl.g1[b] = g1[b]; }
    for (int c = 0; c < 2; ++c) { pl.w0[c] = st.w0[c]; pl.dw[c] = w1[c] - st.w0[c]; }
    pl.pad[0] = pl.pad[1] = 0;
    plans[(size_t)r * kRrSlots + slot] = pl;
    if (op == kReflectEnd) {
        st = ReflectRenderSlot{};   // free
    } else {
        st.held = 1;
        st.d0 = pl.d0 + e;   // what the last output sample used: a == 1 there
        for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = b < bands ? g1[b] : 0.0f;
        st.w0[0] = w1[0];
        st.w0[1] = w1[1];
    }
    it.state->slot[slot] = st;
}

__global__ __launch_bounds__(kRenderTile) void reflect_render_kernel(const ReflectRenderItem* __restrict__ items,
                                                                      const ReflectRenderPlan* __restrict__ plans,
                                                                      const unsigned* __restrict__ n0_all, const float* __restrict__ in_all,
                                                                      float* __restrict__ out_all, int frame, int taps, int bands) {
    __shared__ RenderTaps s_cd;      // of the slot in hand
    __shared__ RenderWindow s_win;   // likewise: every slot has a delay of its own
    const int r = blockIdx.z;
    struct { float* ring; const float* table; unsigned mask; int slots; } it = {items[r].ring, items[r].table, items[r].mask, items[r].slots};
    const int8_t* __restrict__ ops = items[r].op;
    const unsigned n0 = n0_all[r];
    const int ch = blockIdx.y;
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
        const ReflectRenderPlan* __restrict__ plp = plans + (size_t)r * kRrSlots + slot;
        // (the scalars by value, the gain arrays through the record: indexing a copy by the band would put it in scratch)
        struct { float d0, e, w0, dw; } pl = {plp->d0, plp->e, plp->w0[ch], plp->dw[ch]};

        render_build_taps(s_cd, it.table, plp->g0, plp->g1, taps, bands, tid);
        const int i_hi = render_stage_window(s_win, ring, it.mask, in, ch, n0, pl.d0, pl.e, s_a, s_b, frame, frame_f, taps, tid);
        __syncthreads();

        if (live) {
            float a;
            const float y = render_sample(s_cd, s_win, pl.d0, pl.e, s, s_a, i_hi, frame_f, taps, &a);
            const float w = pl.w0 + a * pl.dw;
            out = out + w * y;
        }
        __syncthreads();   // the next slot rebuilds the LDS
    }
    if (!live) return;
    render_store(out_all, ring, it.mask, in, r, ch, n0, s, frame, out);
}

}  // namespace

void launch_reflect_render(const ReflectRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(reflect_render_plan_kernel, dim3((b.count * kRrSlots + tb - 1) / tb), dim3(tb), 0, s, b.items, b.voices, b.plans,
                       b.n0, b.count, b.stride, b.frame, b.bands, b.fs);
    const int tiles = (b.frame + kRenderTile - 1) / kRenderTile;
    hipLaunchKernelGGL(reflect_render_kernel, dim3(tiles, 2, b.count), dim3(kRenderTile), 0, s, b.items, b.plans, b.n0, b.in, b.out, b.frame,
                       b.taps, b.bands);
    if (b.mix) launch_callback_mix(b.out, b.count, b.frame, b.mix, s);
}

}  // namespace fs
