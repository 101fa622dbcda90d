// fs_reflect_render.hip — the early reflections of all rows of one audio callback (fs_reflection_render_process_batch): per source
// a bank of voices, each one the direct renderer's block (fs_direct_render.hip: a time-varying fractional delay and a linear-phase
// FIR whose taps are sum_b gain_b * k_b) reading the source's one history ring, weighted by a ramping per-channel gain and summed
// in ascending slot order.  The reference has no slot for it.
//
// The rule is include/frequensee.h's, to the bit: the file is built with the library's -ffp-contract=off, every fp32 operation
// below rounds on its own, in the order written.  The tap loop is fs_direct_render.hip's and gives its bits.
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
//   mix     one thread per sample, rows in list order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs_internal.hpp"

namespace fs {
namespace {

constexpr int kRrTile = 256;                                   // outputs per workgroup = threads per workgroup
constexpr int kRrMaxTaps = FS_DIRECT_RENDER_MAX_TAPS;
constexpr int kRrSlots = FS_MAX_REFLECTION_VOICES;
// the window of a tile: its outputs, the taps, x(p - 1), and the delay's travel across the tile — the slew limit bounds that
// to half a sample per sample, plus one for the floor
constexpr int kRrWindow = kRrTile + kRrTile / 2 + kRrMaxTaps + 8;

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
    const float half = 0.5f * (float)frame;
    float e = d1 - st.d0;
    if (e < -half) e = -half;
    if (e > half) e = half;
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

__device__ inline float rr_delay(float d0, float e, int s, float frame_f, float* a_out) {
    const float a = (float)(s + 1) / frame_f;
    *a_out = a;
    return d0 + a * e;
}

__global__ __launch_bounds__(kRrTile) void reflect_render_kernel(const ReflectRenderItem* __restrict__ items,
                                                                  const ReflectRenderPlan* __restrict__ plans,
                                                                  const unsigned* __restrict__ n0_all, const float* __restrict__ in_all,
                                                                  float* __restrict__ out_all, int frame, int taps, int bands) {
    __shared__ float2 s_cd[kRrMaxTaps + 1];   // {c0[t], dc[t]} of the slot in hand
    __shared__ float s_win[kRrWindow];
    const int r = blockIdx.z;
    struct { float* ring; const float* table; unsigned mask; int slots; } it = {items[r].ring, items[r].table, items[r].mask, items[r].slots};
    const int8_t* __restrict__ ops = items[r].op;
    const unsigned n0 = n0_all[r];
    const int ch = blockIdx.y;
    const int s_a = blockIdx.x * kRrTile;
    const int s_b = min(s_a + kRrTile, frame) - 1;
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
        const float* __restrict__ g0 = plp->g0;
        const float* __restrict__ g1 = plp->g1;
        struct { float d0, e, w0, dw; } pl = {plp->d0, plp->e, plp->w0[ch], plp->dw[ch]};

        for (int t = tid; t < taps; t += kRrTile) {
            float c0 = 0.0f, c1 = 0.0f;
            for (int b = 0; b < bands; ++b) {
                const float k = it.table[(size_t)b * (size_t)taps + t];
                c0 = c0 + g0[b] * k;
                c1 = c1 + g1[b] * k;
            }
            s_cd[t] = make_float2(c0, c1 - c0);
        }

        // d is monotone in s (every rounding is), so the tile's whole delays lie between those of its first and last output
        float a_unused;
        const int i_a = (int)floorf(rr_delay(pl.d0, pl.e, s_a, frame_f, &a_unused));
        const int i_b = (int)floorf(rr_delay(pl.d0, pl.e, s_b, frame_f, &a_unused));
        const int i_lo = min(i_a, i_b), i_hi = max(i_a, i_b);
        const unsigned p_lo = n0 + (unsigned)s_a - (unsigned)(taps - 1) - (unsigned)i_hi - 1u;   // absolute index of s_win[0]
        const int wlen = min((s_b - s_a) + (i_hi - i_lo) + taps + 1, kRrWindow);
        for (int j = tid; j < wlen; j += kRrTile) {
            const unsigned p = p_lo + (unsigned)j;
            const int rel = (int)(p - n0);   // >= 0: a sample of this block
            float v = 0.0f;
            if (rel < 0) v = ring[p & it.mask];
            else if (rel < frame) v = in[2 * rel + ch];
            s_win[j] = v;
        }
        __syncthreads();

        if (live) {
            float a;
            const float d = rr_delay(pl.d0, pl.e, s, frame_f, &a);
            const float fl = floorf(d);
            const int i = (int)fl;
            const float f = d - fl;
            // tap t reads x(p) = s_win[base - t] and x(p - 1) = s_win[base - t - 1], p = n0 + s - t - i
            const int base = min((s - s_a) + (i_hi - i) + taps, kRrWindow - 1);
            float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
            float xp = s_win[base];
            int t = 0;
            for (; t + 4 <= taps; t += 4) {
                const float2 k0 = s_cd[t], k1 = s_cd[t + 1], k2 = s_cd[t + 2], k3 = s_cd[t + 3];
                const float x1 = s_win[base - t - 1], x2 = s_win[base - t - 2], x3 = s_win[base - t - 3], x4 = s_win[base - t - 4];
                acc0 = acc0 + (k0.x + a * k0.y) * (xp + f * (x1 - xp));
                acc1 = acc1 + (k1.x + a * k1.y) * (x1 + f * (x2 - x1));
                acc2 = acc2 + (k2.x + a * k2.y) * (x2 + f * (x3 - x2));
                acc3 = acc3 + (k3.x + a * k3.y) * (x3 + f * (x4 - x3));
                xp = x4;
            }
            if (t < taps) {
                const float2 k0 = s_cd[t];
                const float x1 = s_win[base - t - 1];
                acc0 = acc0 + (k0.x + a * k0.y) * (xp + f * (x1 - xp));
                xp = x1;
                ++t;
            }
            if (t < taps) {
                const float2 k1 = s_cd[t];
                const float x2 = s_win[base - t - 1];
                acc1 = acc1 + (k1.x + a * k1.y) * (xp + f * (x2 - xp));
                xp = x2;
                ++t;
            }
            if (t < taps) {
                const float2 k2 = s_cd[t];
                const float x3 = s_win[base - t - 1];
                acc2 = acc2 + (k2.x + a * k2.y) * (xp + f * (x3 - xp));
            }
            const float y = (acc0 + acc1) + (acc2 + acc3);
            const float w = pl.w0 + a * pl.dw;
            out = out + w * y;
        }
        __syncthreads();   // the next slot rebuilds the LDS
    }
    if (!live) return;
    out_all[(size_t)r * 2 * (size_t)frame + 2 * (size_t)s + ch] = out;
    ring[(n0 + (unsigned)s) & it.mask] = in[2 * s + ch];
}

// mix[j] = ((out[0][j] + out[1][j]) + out[2][j]) + ... in list order, fp32: one thread per sample, so the order is fixed
__global__ void reflect_render_mix_kernel(const float* __restrict__ out_all, int count, int n2, float* __restrict__ mix) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n2) return;
    float v = out_all[j];
    for (int r = 1; r < count; ++r) v = v + out_all[(size_t)r * (size_t)n2 + j];
    mix[j] = v;
}

}  // namespace

void launch_reflect_render(const ReflectRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(reflect_render_plan_kernel, dim3((b.count * kRrSlots + tb - 1) / tb), dim3(tb), 0, s, b.items, b.voices, b.plans,
                       b.n0, b.count, b.stride, b.frame, b.bands, b.fs);
    const int tiles = (b.frame + kRrTile - 1) / kRrTile;
    hipLaunchKernelGGL(reflect_render_kernel, dim3(tiles, 2, b.count), dim3(kRrTile), 0, s, b.items, b.plans, b.n0, b.in, b.out, b.frame,
                       b.taps, b.bands);
    if (b.mix)
        hipLaunchKernelGGL(reflect_render_mix_kernel, dim3((2 * b.frame + tb - 1) / tb), dim3(tb), 0, s, b.out, b.count, 2 * b.frame, b.mix);
}

}  // namespace fs
