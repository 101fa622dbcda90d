// fs_ambisonic_render.hip — the ambisonic voices of all rows of one audio callback (fs_ambisonic_render_process_batch): per source
// a bank of voices as the reflection renderer's (fs_reflect_render.hip), each a MONO voice — the source's downmix through the
// voice's delay and band FIR — fanned out to the C = (order + 1)^2 channels of an ambisonic bus (ACN order, SN3D normalisation)
// by ramping channel gains the plan pass computes from the voice's gain and direction.  The reference has no slot for it.
//
// The rule is include/frequensee.h's, to the bit: the file is built with the library's -ffp-contract=off, every fp32 operation
// rounds on its own, in the order written.  The voice's block and the plan pass are fs_dev_render.hpp's, the one text the render
// kernels are built from; this file says what an ambisonic voice carries beyond a delay and band gains — C channel gains, encoded
// by fs_internal.hpp's ambisonic_encode, the very function fs_ambisonic_encode runs on the host — and holds a render pass of its
// own: voice_bank_render evaluates a voice once per output channel, this one evaluates it ONCE and weights it C times.
//
// Which slot continues, ends or starts is decided on the host (VoiceBankItem::op); three launches, whatever the number of rows:
//   plan    one thread per (row, slot): voice_bank_plan with the C channel gains g * Y_c(direction) as the aim.
//   render  a grid of (frame / 256 output tiles) x rows, templated on C: per sounding slot, ascending, the taps {c0[t], dc[t]} and
//           the tile's read window (the mono ring, then the block's downmix) into LDS, one tap loop per thread, then C
//           multiply-adds into C register accumulators — the slot's {w0[c], dw[c]} are read through the plan record, whose address
//           is the workgroup's: scalar loads.  After the last slot a thread stores its C contiguous floats straight from the
//           registers (one 16-byte store at C = 4, four at C = 16, no LDS transpose: DESIGN.md section 8, "Ambisonic voices") and
//           appends its downmixed input sample to the ring.
//   mix     one thread per sample, rows in list order (launch_callback_mix, fs_reverb.hip: the audio callbacks' one mix).
#include "fs_dev_render.hpp"

namespace fs {
namespace {

struct AmbisonicVoices {
    struct Aim { float w[kAmbisonicChannels]; };   // the channel gains; 0 beyond C
    static __device__ __forceinline__ Aim read(const fs_ambisonic_voice& v, int order) {
        float y[kAmbisonicChannels];
        ambisonic_encode(order, v.direction, y);
        const int channels = (order + 1) * (order + 1);
        Aim aim;
        for (int c = 0; c < kAmbisonicChannels; ++c) aim.w[c] = c < channels ? v.gain * y[c] : 0.0f;
        return aim;
    }
    static __device__ __forceinline__ Aim fade_out(const AmbisonicRenderSlot&) { return Aim{}; }
    static __device__ __forceinline__ void from_silence(AmbisonicRenderSlot& st, const Aim&) {
        for (int c = 0; c < kAmbisonicChannels; ++c) st.w0[c] = 0.0f;
    }
    static __device__ __forceinline__ void plan(AmbisonicRenderPlan& pl, const AmbisonicRenderSlot& st, const Aim& aim, const AmbisonicRenderItem&,
                                                int) {
        for (int c = 0; c < kAmbisonicChannels; ++c) { pl.w0[c] = st.w0[c]; pl.dw[c] = aim.w[c] - st.w0[c]; }
        for (int& p : pl.pad) p = 0;
    }
    static __device__ __forceinline__ void keep(AmbisonicRenderSlot& st, const Aim& aim) {
        for (int c = 0; c < kAmbisonicChannels; ++c) st.w0[c] = aim.w[c];
    }
};

__global__ void ambisonic_render_plan_kernel(const AmbisonicRenderItem* __restrict__ items, const fs_ambisonic_voice* __restrict__ voices,
                                             AmbisonicRenderPlan* __restrict__ plans, unsigned* __restrict__ n0_out, int count, int stride,
                                             int frame, int bands, float fs_f, int order) {
    voice_bank_plan<AmbisonicVoices>(items, voices, plans, n0_out, count, stride, frame, bands, fs_f, order);
}

// The render pass.  As in voice_bank_render the trip count and every branch around a barrier depend on the row only, and a thread
// past the frame's end keeps filling tables and windows and skips only the tap loop and the stores.
template <int C>
__global__ __launch_bounds__(kRenderTile) void ambisonic_render_kernel(const AmbisonicRenderItem* __restrict__ items,
                                                                        const AmbisonicRenderPlan* __restrict__ plans,
                                                                        const unsigned* __restrict__ n0_all, const float* __restrict__ in_all,
                                                                        float* __restrict__ out_all, int frame, int taps, int bands) {
    __shared__ RenderTaps s_cd;      // of the slot in hand
    __shared__ RenderWindow s_win;   // likewise: every slot has a delay of its own
    const int r = blockIdx.y;
    struct { float* ring; const float* table; unsigned mask; int slots; } it = {items[r].ring, items[r].table, items[r].mask, items[r].slots};
    const int8_t* __restrict__ ops = items[r].op;
    const unsigned n0 = n0_all[r];
    const int s_a = blockIdx.x * kRenderTile;
    const int s_b = min(s_a + kRenderTile, frame) - 1;
    const int tid = threadIdx.x;
    const int s = s_a + tid;
    const bool live = s < frame;
    const RenderDownmix x_in = {in_all + (size_t)r * 2 * (size_t)frame};
    const float frame_f = (float)frame;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;

    for (int slot = 0; slot < it.slots; ++slot) {   // (uniform over the workgroup: the row's)
        if (ops[slot] == kVoiceIdle) continue;
        const AmbisonicRenderPlan* __restrict__ plp = plans + (size_t)r * kVoiceSlots + slot;
        const float d0 = plp->d0, e = plp->e;
        // At C <= 4 the slot's weights by value, here, as voice_bank_render reads its pair: read where they are used, their scalar
        // loads' latency stands between the tap loop and the slot's closing barrier, once per slot.  At C = 9 and 16 they stay
        // where they are used: 2 C more scalar registers would not fit across the tap loop.
        constexpr int kEarly = C <= 4 ? C : 0;
        float w0[kEarly + 1], dw[kEarly + 1];
#pragma unroll
        for (int c = 0; c < kEarly; ++c) { w0[c] = plp->w0[c]; dw[c] = plp->dw[c]; }

        render_build_taps(s_cd, it.table, plp->g0, plp->g1, taps, bands, tid);
        const int i_hi = render_stage_window(s_win, it.ring, it.mask, x_in, n0, d0, e, s_a, s_b, frame, frame_f, taps, tid);
        __syncthreads();

        if (live) {
            float a;
            const float y = render_sample(s_cd, s_win, d0, e, s, s_a, i_hi, frame_f, taps, &a);
#pragma unroll
            for (int c = 0; c < C; ++c) {   // (the constant index after unrolling: registers, and scalar loads of the record)
                const float w = c < kEarly ? w0[c] + a * dw[c] : plp->w0[c] + a * plp->dw[c];
                acc[c] = acc[c] + w * y;
            }
        }
        __syncthreads();   // the next slot rebuilds the LDS
    }
    if (!live) return;
    float* __restrict__ dst = out_all + ((size_t)r * (size_t)frame + (size_t)s) * C;
    if constexpr (C % 4 == 0) {   // (rows of C * frame floats behind a 256-byte aligned base: 16-byte aligned)
#pragma unroll
        for (int c = 0; c < C; c += 4) *reinterpret_cast<float4*>(dst + c) = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = acc[c];
    }
    render_append(it.ring, it.mask, x_in, n0, s);
}

}  // namespace

void launch_ambisonic_render(const AmbisonicRenderBatch& b, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(ambisonic_render_plan_kernel, dim3((b.count * kVoiceSlots + tb - 1) / tb), dim3(tb), 0, s, b.items, b.voices, b.plans,
                       b.n0, b.count, b.stride, b.frame, b.bands, b.fs, b.order);
    const dim3 grid((b.frame + kRenderTile - 1) / kRenderTile, b.count);
    const int channels = (b.order + 1) * (b.order + 1);
    auto render = b.order == 0 ? ambisonic_render_kernel<1> : b.order == 1 ? ambisonic_render_kernel<4> :
                  b.order == 2 ? ambisonic_render_kernel<9> : ambisonic_render_kernel<16>;
    hipLaunchKernelGGL(render, grid, dim3(kRenderTile), 0, s, b.items, b.plans, b.n0, b.in, b.out, b.frame, b.taps, b.bands);
    if (b.mix) launch_callback_mix(b.out, b.count, channels * b.frame, b.mix, s);
}

}  // namespace fs
