// fs_reflect_render.hip — the early reflections of all rows of one audio callback (fs_reflection_render_process_batch): per source
// a bank of voices, each one the direct renderer's block (fs_direct_render.hip: a time-varying fractional delay and a linear-phase
// FIR whose taps are sum_b gain_b * k_b) reading the source's one history ring, weighted by a ramping per-channel gain and summed
// in ascending slot order.  The reference has no slot for it.
//
// The rule is include/frequensee.h's, to the bit: the file is built with the library's -ffp-contract=off, every fp32 operation
// rounds on its own, in the order written.  The voice's block and the voice bank's two passes are fs_dev_render.hpp's, the one text
// the render kernels are built from; this file says what a reflection voice carries beyond a delay and band gains — a pair of
// channel gains — and that its taps are built from the row's band table.
//
// Which slot continues, ends or starts is decided on the host (VoiceBankItem::op); three launches, whatever the number of rows:
//   plan    one thread per (row, slot): voice_bank_plan with the channel gains as the aim.
//   render  a grid of (frame / 256 output tiles) x 2 channels x rows: voice_bank_render, which per slot builds the taps
//           {c0[t], dc[t]} from the band table and the slot's gains and weights the slot by channel ch's ramping gain.
//   mix     one thread per sample, rows in list order (launch_callback_mix, fs_reverb.hip: the audio callbacks' one mix).
#include "fs_dev_render.hpp"

namespace fs {
namespace {

struct ReflectVoices {
    struct Aim { float w[2]; };   // the channel gains
    static __device__ __forceinline__ Aim read(const fs_reflection_voice& v) { return {{v.channel_gain[0], v.channel_gain[1]}}; }
    static __device__ __forceinline__ Aim fade_out(const ReflectRenderSlot&) { return {{0.0f, 0.0f}}; }
    static __device__ __forceinline__ void from_silence(ReflectRenderSlot& st, const Aim&) { st.w0[0] = st.w0[1] = 0.0f; }
    static __device__ __forceinline__ void plan(ReflectRenderPlan& pl, const ReflectRenderSlot& st, const Aim& aim, const ReflectRenderItem&, int) {
        for (int c = 0; c < 2; ++c) { pl.w0[c] = st.w0[c]; pl.dw[c] = aim.w[c] - st.w0[c]; }
        pl.pad[0] = pl.pad[1] = 0;
    }
    static __device__ __forceinline__ void keep(ReflectRenderSlot& st, const Aim& aim) {
        st.w0[0] = aim.w[0];
        st.w0[1] = aim.w[1];
    }
};

__global__ void reflect_render_plan_kernel(const ReflectRenderItem* __restrict__ items, const fs_reflection_voice* __restrict__ voices,
                                           ReflectRenderPlan* __restrict__ plans, unsigned* __restrict__ n0_out, int count, int stride,
                                           int frame, int bands, float fs_f) {
    voice_bank_plan<ReflectVoices>(items, voices, plans, n0_out, count, stride, frame, bands, fs_f);
}

__global__ __launch_bounds__(kRenderTile) void reflect_render_kernel(const ReflectRenderItem* __restrict__ items,
                                                                      const ReflectRenderPlan* __restrict__ plans,
                                                                      const unsigned* __restrict__ n0_all, const float* __restrict__ in_all,
                                                                      float* __restrict__ out_all, int frame, int taps, int bands) {
    voice_bank_render(
        items, plans, n0_all, in_all, out_all, frame, taps,
        [=](RenderTaps& s_cd, const float* __restrict__ table, const ReflectRenderPlan* __restrict__ plp, int, int tid) {
            render_build_taps(s_cd, table, plp->g0, plp->g1, taps, bands, tid);
        },
        [](const ReflectRenderPlan* __restrict__ plp, int ch) { return make_float2(plp->w0[ch], plp->dw[ch]); });
}

}  // namespace

void launch_reflect_render(const ReflectRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(reflect_render_plan_kernel, dim3((b.count * kVoiceSlots + tb - 1) / tb), dim3(tb), 0, s, b.items, b.voices, b.plans,
                       b.n0, b.count, b.stride, b.frame, b.bands, b.fs);
    const int tiles = (b.frame + kRenderTile - 1) / kRenderTile;
    hipLaunchKernelGGL(reflect_render_kernel, dim3(tiles, 2, b.count), dim3(kRenderTile), 0, s, b.items, b.plans, b.n0, b.in, b.out, b.frame,
                       b.taps, b.bands);
    if (b.mix) launch_callback_mix(b.out, b.count, 2 * b.frame, b.mix, s);
}

}  // namespace fs
