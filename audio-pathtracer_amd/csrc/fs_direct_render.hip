// fs_direct_render.hip — the direct sound of all rows of one audio callback (fs_direct_render_process_batch): per source a
// time-varying fractional delay (which is also the Doppler shift) and a short linear-phase FIR whose taps are
// sum_b gain_b * k_b, k_b the band kernels of fs_direct_band_kernels.  The reference leaves this slot empty
// (FFrequenSeeAudioOcclusionPlugin::ProcessAudio fetches the occlusion scalar and keeps the multiply commented out).
//
// The rule is include/frequensee.h's, to the bit: the file is built with the library's -ffp-contract=off, every fp32 operation
// below rounds on its own, in the order written.
//
// Three launches, whatever the number of rows:
//   plan    one thread per row: reads the source's device-resident state (n0, d0, g0, primed), fixes what this callback ramps
//           from and by how much (the slew limit) in the row's plan record, and writes the state the callback leaves behind.
//   render  a grid of (frame / 256 output tiles) x 2 channels x rows; a workgroup finds its row through blockIdx.z.  It builds
//           the row's taps c0[t] and their change dc[t] in LDS, stages the tile's read window (history ring + this block) in
//           LDS, and every thread runs the four-accumulator tap loop of one output sample out of LDS: c0 / dc are wave-uniform
//           broadcasts, neighbouring lanes read neighbouring samples, x(p - 1) of tap t is x(p) of tap t + 1 (one sample read
//           per tap).  The thread then appends its input sample to the ring: a callback reads ring positions
//           [n0 - D - T, n0) and writes [n0, n0 + F), disjoint modulo the ring because the ring holds D + T + 1 + F or more.
//   mix     one thread per sample, rows in list order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs_internal.hpp"

namespace fs {
namespace {

constexpr int kDrTile = 256;                                   // outputs per workgroup = threads per workgroup
constexpr int kDrMaxTaps = FS_DIRECT_RENDER_MAX_TAPS;
// the window of a tile: its outputs, the taps, x(p - 1), and the delay's travel across the tile — the slew limit bounds that
// to half a sample per sample, plus one for the floor
constexpr int kDrWindow = kDrTile + kDrTile / 2 + kDrMaxTaps + 8;

__global__ void direct_render_plan_kernel(const DirectRenderItem* __restrict__ items, DirectRenderPlan* __restrict__ plans, int count,
                                          int frame, int bands) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= count) return;
    const DirectRenderItem it = items[r];
    DirectRenderState st = *it.state;
    DirectRenderPlan pl;
    pl.n0 = st.n0;
    pl.d0 = st.primed ? st.d0 : it.d1;
    for (int b = 0; b < FS_MAX_BANDS; ++b) pl.g0[b] = st.primed ? st.g0[b] : it.g1[b];
    const float half = 0.5f * (float)frame;
    float e = it.d1 - pl.d0;
    if (e < -half) e = -half;
    if (e > half) e = half;
    pl.e = e;
    pl.pad = 0;
    plans[r] = pl;
    st.n0 = pl.n0 + (unsigned)frame;
    st.d0 = pl.d0 + e;   // what the last output sample used: a == 1 there
    st.primed = 1;
    for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = b < bands ? it.g1[b] : 0.0f;
    *it.state = st;
}

__device__ inline float dr_delay(float d0, float e, int s, float frame_f, float* a_out) {
    const float a = (float)(s + 1) / frame_f;
    *a_out = a;
    return d0 + a * e;
}

__global__ __launch_bounds__(kDrTile) void direct_render_kernel(const DirectRenderItem* __restrict__ items,
                                                                 const DirectRenderPlan* __restrict__ plans,
                                                                 const float* __restrict__ in_all, float* __restrict__ out_all, int frame,
                                                                 int taps, int bands) {
    __shared__ float2 s_cd[kDrMaxTaps + 1];   // {c0[t], dc[t]}
    __shared__ float s_win[kDrWindow];
    const int r = blockIdx.z;
    // (the scalars by value, the gain arrays through the tables: indexing a copy by the band would put it in scratch)
    const float* __restrict__ g0 = plans[r].g0;
    const float* __restrict__ g1 = items[r].g1;
    struct { float* ring; const float* table; unsigned mask; } it = {items[r].ring, items[r].table, items[r].mask};
    struct { unsigned n0; float d0, e; } pl = {plans[r].n0, plans[r].d0, plans[r].e};
    const int ch = blockIdx.y;
    const int s_a = blockIdx.x * kDrTile;
    const int s_b = min(s_a + kDrTile, frame) - 1;
    const int tid = threadIdx.x;
    const float* __restrict__ in = in_all + (size_t)r * 2 * (size_t)frame;
    float* __restrict__ ring = it.ring + (size_t)ch * ((size_t)it.mask + 1);
    const float frame_f = (float)frame;

    for (int t = tid; t < taps; t += kDrTile) {
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
    const int i_a = (int)floorf(dr_delay(pl.d0, pl.e, s_a, frame_f, &a_unused));
    const int i_b = (int)floorf(dr_delay(pl.d0, pl.e, s_b, frame_f, &a_unused));
    const int i_lo = min(i_a, i_b), i_hi = max(i_a, i_b);
    const unsigned p_lo = pl.n0 + (unsigned)s_a - (unsigned)(taps - 1) - (unsigned)i_hi - 1u;   // absolute index of s_win[0]
    const int wlen = min((s_b - s_a) + (i_hi - i_lo) + taps + 1, kDrWindow);
    for (int j = tid; j < wlen; j += kDrTile) {
        const unsigned p = p_lo + (unsigned)j;
        const int rel = (int)(p - pl.n0);   // >= 0: a sample of this block
        float v = 0.0f;
        if (rel < 0) v = ring[p & it.mask];
        else if (rel < frame) v = in[2 * rel + ch];
        s_win[j] = v;
    }
    __syncthreads();

    const int s = s_a + tid;
    if (s >= frame) return;
    float a;
    const float d = dr_delay(pl.d0, pl.e, s, frame_f, &a);
    const float fl = floorf(d);
    const int i = (int)fl;
    const float f = d - fl;
    // tap t reads x(p) = s_win[base - t] and x(p - 1) = s_win[base - t - 1], p = n0 + s - t - i
    const int base = min((s - s_a) + (i_hi - i) + taps, kDrWindow - 1);
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
    out_all[(size_t)r * 2 * (size_t)frame + 2 * (size_t)s + ch] = (acc0 + acc1) + (acc2 + acc3);
    ring[(pl.n0 + (unsigned)s) & it.mask] = in[2 * s + ch];
}

// mix[j] = ((out[0][j] + out[1][j]) + out[2][j]) + ... in list order, fp32: one thread per sample, so the order is fixed
__global__ void direct_render_mix_kernel(const float* __restrict__ out_all, int count, int n2, float* __restrict__ mix) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n2) return;
    float v = out_all[j];
    for (int r = 1; r < count; ++r) v = v + out_all[(size_t)r * (size_t)n2 + j];
    mix[j] = v;
}

}  // namespace

void launch_direct_render(const DirectRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(direct_render_plan_kernel, dim3((b.count + tb - 1) / tb), dim3(tb), 0, s, b.items, b.plans, b.count, b.frame, b.bands);
    const int tiles = (b.frame + kDrTile - 1) / kDrTile;
    hipLaunchKernelGGL(direct_render_kernel, dim3(tiles, 2, b.count), dim3(kDrTile), 0, s, b.items, b.plans, b.in, b.out, b.frame, b.taps,
                       b.bands);
    if (b.mix)
        hipLaunchKernelGGL(direct_render_mix_kernel, dim3((2 * b.frame + tb - 1) / tb), dim3(tb), 0, s, b.out, b.count, 2 * b.frame, b.mix);
}

}  // namespace fs
