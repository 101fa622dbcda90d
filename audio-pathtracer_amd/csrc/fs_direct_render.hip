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
//   render  a grid of (frame / 256 output tiles) x 2 channels x rows; a workgroup finds its row through blockIdx.z.  One voice per
//           row, its state in the plan record: the pieces of fs_dev_render.hpp (shared with fs_reflect_render.hip) in a row — the
//           row's taps c0[t] and their change dc[t] and the tile's read window (history ring + this block) into LDS, one barrier,
//           then every thread of the frame runs the tap loop of one output sample out of LDS, stores it and appends its input
//           sample to the ring; a thread past the frame's end leaves behind the barrier.
//   mix     one thread per sample, rows in list order (launch_callback_mix, fs_reverb.hip: the three callbacks' one mix).
#include "fs_dev_render.hpp"

namespace fs {
namespace {

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
    const float e = render_slew(it.d1 - pl.d0, frame);
    pl.e = e;
    pl.pad = 0;
    plans[r] = pl;
    st.n0 = pl.n0 + (unsigned)frame;
    st.d0 = pl.d0 + e;   // what the last output sample used: a == 1 there
    st.primed = 1;
    for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = b < bands ? it.g1[b] : 0.0f;
    *it.state = st;
}

__global__ __launch_bounds__(kRenderTile) void direct_render_kernel(const DirectRenderItem* __restrict__ items,
                                                                     const DirectRenderPlan* __restrict__ plans,
                                                                     const float* __restrict__ in_all, float* __restrict__ out_all, int frame,
                                                                     int taps, int bands) {
    __shared__ RenderTaps s_cd;
    __shared__ RenderWindow s_win;
    const int r = blockIdx.z;
    // (the scalars by value, the gain arrays through the tables: indexing a copy by the band would put it in scratch)
    const float* __restrict__ g0 = plans[r].g0;
    const float* __restrict__ g1 = items[r].g1;
    struct { float* ring; const float* table; unsigned mask; } it = {items[r].ring, items[r].table, items[r].mask};
    struct { unsigned n0; float d0, e; } pl = {plans[r].n0, plans[r].d0, plans[r].e};
    const int ch = blockIdx.y;
    const int s_a = blockIdx.x * kRenderTile;
    const int s_b = min(s_a + kRenderTile, frame) - 1;
    const int tid = threadIdx.x;
    const float* __restrict__ in = in_all + (size_t)r * 2 * (size_t)frame;
    float* __restrict__ ring = it.ring + (size_t)ch * ((size_t)it.mask + 1);
    const float frame_f = (float)frame;

    render_build_taps(s_cd, it.table, g0, g1, taps, bands, tid);
    const int i_hi = render_stage_window(s_win, ring, it.mask, in, ch, pl.n0, pl.d0, pl.e, s_a, s_b, frame, frame_f, taps, tid);
    __syncthreads();   // the one barrier: nothing rebuilds the LDS

    const int s = s_a + tid;
    if (s >= frame) return;
    float a;
    const float y = render_sample(s_cd, s_win, pl.d0, pl.e, s, s_a, i_hi, frame_f, taps, &a);
    render_store(out_all, ring, it.mask, in, r, ch, pl.n0, s, frame, y);
}

}  // namespace

void launch_direct_render(const DirectRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(direct_render_plan_kernel, dim3((b.count + tb - 1) / tb), dim3(tb), 0, s, b.items, b.plans, b.count, b.frame, b.bands);
    const int tiles = (b.frame + kRenderTile - 1) / kRenderTile;
    hipLaunchKernelGGL(direct_render_kernel, dim3(tiles, 2, b.count), dim3(kRenderTile), 0, s, b.items, b.plans, b.in, b.out, b.frame, b.taps,
                       b.bands);
    if (b.mix) launch_callback_mix(b.out, b.count, 2 * b.frame, b.mix, s);
}

}  // namespace fs
