// fs_reverb.hip — row f2, the reverb plugin's per-callback convolution (FFrequenSeeAudioReverbPlugin::ProcessSourceAudio,
// FrequenSeeAudioReverbPlugin.cpp:118-170, ConvolveFFT :172-213), for all rows of one audio callback as one set of launches
// (fs_reverb_process_batch; fs_reverb_process is a callback of one row).  This is the DIRECT engine, the default; a source may
// choose the partitioned one of fs_reverb_part.hip instead (fs_reverb_set_engine), and a call may hold rows of both.
//
// The reference zero-pads the last 47 999 + 1 024 samples and the 48 000-tap IR to 65 536 and multiplies three KissFFT spectra;
// only output samples [47 999, 49 023) are kept, for which the circular product equals the plain convolution
//   out[s] = sum_k IR[k] * u[47 999 + s - k].
// On this chip 2 x 1024 x 48 000 MACs are a few microseconds of fp32 FMA, so the kernel evaluates that sum directly (no FFT, no
// 65 536-point scratch, deterministic order): thread t owns a contiguous 192-tap slice and slides a 31-sample register window
// over it (47 loads per 256 FMAs), partial sums meet in LDS.
//
// Every kernel takes a table of per-row descriptors (ReverbItem, fs_internal.hpp) and lays the rows side by side: the convolution
// is a grid of (frame / 16 output tiles) x 2 channels x rows, a workgroup finds its row through blockIdx.z (one row alone is 128
// workgroups on a chip of 256 CUs).  The file is built with the library's -ffp-contract=off: the fade mix (1 - g) acc + g acc_to
// and (p + 1) / L round operation by operation.
//
// Rows that fade (two IRs, 16 more accumulators) and rows that do not are two launches over two index lists: one kernel
// with a workgroup-uniform branch would give every workgroup the fading one's registers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs_internal.hpp"

namespace fs {
namespace {

constexpr int kRevOut = 16;      // outputs per workgroup
constexpr int kRevRing = 65536;  // history ring length per channel (power of two >= 47 999)
static_assert(kRevRing == kReverbRing, "the kernels' ring is the host's");

// A crossfade starts for the rows of `take` (fs_reverb_set_crossfade): h_from := (1 - a) h_from + a h_to — the IR heard at the last
// output sample of a fade that is cut short (a = p0 / L; a = 0 leaves h_from as it is) — then h_to := the device-resident IR.
__global__ void reverb_batch_fade_start_kernel(const ReverbItem* __restrict__ items, const int* __restrict__ take, int n) {
    const ReverbItem it = items[take[blockIdx.y]];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* __restrict__ h_from = it.take_from;
    float* __restrict__ h_to = it.take_to;
    const float a = it.take_a;
    if (a > 0.0f) h_from[i] = (1.0f - a) * h_from[i] + a * h_to[i];
    h_to[i] = it.take_ir[i];
}

// Row r of the call (blockIdx.y), the passes of `mode` (a convolved row of the partitioned engine has neither tails nor a ring of
// this kind: fs_reverb_part.hip serves it).  kRevTails: a bypassed row (apply == 0) gets out row := in row (what the
// mix sums; the host copies the row itself), a convolved one the two mono tails of this callback.  kRevPush: a convolved row's
// samples enter its history ring.
constexpr int kRevTails = 1, kRevPush = 2;
__global__ void reverb_batch_prepare_kernel(const ReverbItem* __restrict__ items, const float* __restrict__ in_all,
                                            float* __restrict__ cur_all, float* __restrict__ out_all, int frame, int literal, int mode) {
    const int r = blockIdx.y;
    const ReverbItem it = items[r];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= frame) return;
    const float* in = in_all + (size_t)r * 2 * (size_t)frame;
    if (!it.apply) {
        if (mode & kRevTails) {
            float* out = out_all + (size_t)r * 2 * (size_t)frame;
            out[2 * i] = in[2 * i];
            out[2 * i + 1] = in[2 * i + 1];
        }
        return;
    }
    if (it.engine != FS_REVERB_ENGINE_DIRECT) return;
    if (mode & kRevTails) {
        float* cur = cur_all + (size_t)r * 2 * (size_t)frame;
        // RVB.cpp:147-148 copies the first `frame` floats of the INTERLEAVED buffer into both mono tails
        cur[i] = literal ? in[i] : in[2 * i];
        cur[frame + i] = literal ? in[i] : in[2 * i + 1];
    }
    if (mode & kRevPush) {
        // AudioTailBuffer{Left,Right}.AddSamples(in, frame, ch, 2)  RVB.cpp:144-145
        float* ring = it.ring;
        ring[(it.head + (unsigned)i) & (unsigned)(kRevRing - 1)] = in[2 * i];
        ring[kRevRing + ((it.head + (unsigned)i) & (unsigned)(kRevRing - 1))] = in[2 * i + 1];
    }
}

// The convolution of row list[blockIdx.z]:  out[s] = sum_k IR[k] * u[tail + s - k],
//   u[j] = j < tail ? ring[(head - tail + j) & mask] : cur[j - tail]
// thread t owns a contiguous 16-aligned tap slice and slides a 31-sample register window over it, partial sums meet in LDS.
// FADE (fs_reverb_set_crossfade, its own instantiation): a second IR `ir_to` over the same register window — the u loads are
// shared, the IR loads and FMAs double — and per output y = (1 - g) (ir * u) + g (ir_to * u), g = (p + 1) / fade_len while
// p = fade_pos + s < fade_len, else 1.  g depends on the output only, so each thread mixes its partial sums before the reduction
// (the sum is linear).
template <bool FADE>
__global__ __launch_bounds__(kBlock) void reverb_batch_conv_kernel(const ReverbItem* __restrict__ items, const int* __restrict__ list,
                                                                   int ir_size, const float* __restrict__ cur_all, int frame,
                                                                   float* __restrict__ out_all) {
    __shared__ float s_part[kRevOut][kBlock + 1];
    const int r = list[blockIdx.z];
    const ReverbItem it = items[r];
    const float* __restrict__ ir = it.ir;
    const float* __restrict__ ir_to = it.ir_to;
    const unsigned head = it.head;
    const int fade_pos = it.fade_pos, fade_len = it.fade_len;
    float* __restrict__ out_interleaved = out_all + (size_t)r * 2 * (size_t)frame;
    const int ch = blockIdx.y;
    const int s0 = blockIdx.x * kRevOut;
    const int tail = ir_size - 1;
    const float* __restrict__ rg = it.ring + (size_t)ch * kRevRing;
    const float* __restrict__ cu = cur_all + (size_t)r * 2 * (size_t)frame + (size_t)ch * frame;
    const unsigned base = head - (unsigned)tail;   // ring index of u[0]
    const int slice = ((ir_size + kBlock - 1) / kBlock + 15) & ~15;
    const int k0 = (int)threadIdx.x * slice;
    const int k1 = min(k0 + slice, ir_size);
    float acc[kRevOut], acc_to[kRevOut];
#pragma unroll
    for (int o = 0; o < kRevOut; ++o) { acc[o] = 0.0f; acc_to[o] = 0.0f; }
    for (int kb = k0; kb < k1; kb += 16) {
        float w[31], h[16];
        const int j0 = tail + s0 - kb - 15;   // u index of w[0]
#pragma unroll
        for (int i = 0; i < 31; ++i) {
            const int j = j0 + i;
            float v = 0.0f;
            if (j >= 0 && j < tail + frame) v = j < tail ? rg[(base + (unsigned)j) & (unsigned)(kRevRing - 1)] : cu[j - tail];
            w[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) h[i] = (kb + i) < ir_size ? ir[kb + i] : 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int o = 0; o < kRevOut; ++o) acc[o] = fmaf(h[i], w[15 - i + o], acc[o]);
        if (FADE) {
            float h2[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) h2[i] = (kb + i) < ir_size ? ir_to[kb + i] : 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i)
#pragma unroll
                for (int o = 0; o < kRevOut; ++o) acc_to[o] = fmaf(h2[i], w[15 - i + o], acc_to[o]);
        }
    }
    if (FADE) {
#pragma unroll
        for (int o = 0; o < kRevOut; ++o) {
            const int p = fade_pos + s0 + o;
            const float g = p < fade_len ? (float)(p + 1) / (float)fade_len : 1.0f;
            acc[o] = (1.0f - g) * acc[o] + g * acc_to[o];
        }
    }
#pragma unroll
    for (int o = 0; o < kRevOut; ++o) s_part[o][threadIdx.x] = acc[o];
    __syncthreads();
    for (int stride = kBlock / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride)
#pragma unroll
            for (int o = 0; o < kRevOut; ++o) s_part[o][threadIdx.x] += s_part[o][threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x < kRevOut && s0 + (int)threadIdx.x < frame) {
        float v = s_part[threadIdx.x][0];
        v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);                 // FMath::Clamp RVB.cpp:165-167, MixAlpha = 1
        out_interleaved[2 * (s0 + (int)threadIdx.x) + ch] = v;
    }
}

// mix[j] = ((out[0][j] + out[1][j]) + out[2][j]) + ... in list order, fp32, not clamped: one thread per sample, so the order is fixed
__global__ void callback_mix_kernel(const float* __restrict__ out_all, int count, int n2, float* __restrict__ mix) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n2) return;
    float v = out_all[j];
    for (int r = 1; r < count; ++r) v = v + out_all[(size_t)r * (size_t)n2 + j];
    mix[j] = v;
}

}  // namespace

void launch_callback_mix(const float* out, int count, int row, float* mix, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(callback_mix_kernel, dim3((row + tb - 1) / tb), dim3(tb), 0, s, out, count, row, mix);
}

void launch_reverb_batch_fade_start(const ReverbItem* items, const int* take, int n_take, int n, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(reverb_batch_fade_start_kernel, dim3((n + tb - 1) / tb, n_take), dim3(tb), 0, s, items, take, n);
}

void launch_reverb_batch(const ReverbBatch& b, hipStream_t s) {
    const int tb = 256;
    const dim3 rows((b.frame + tb - 1) / tb, b.count);
    // A callback appends ring positions [head, head + frame) and its convolution reads [head - tail, head), tail = ir_size - 1,
    // both modulo kRevRing: they are disjoint exactly while tail + frame <= kRevRing, and then the push rides in the prepare pass
    // in front of the convolution (the default IR with any legal frame: 47 999 + 16 384 = 64 383 <= 65 536).  A longer IR's
    // appended samples would land on the oldest history the convolution is about to read: there the push runs behind it.
    const bool fused = (b.ir_size - 1) + b.frame <= kRevRing;
    if (b.n_direct > 0)   // (a call of partitioned rows alone has nothing to prepare)
        hipLaunchKernelGGL(reverb_batch_prepare_kernel, rows, dim3(tb), 0, s, b.items, b.in, b.cur, b.out, b.frame, b.literal_tail,
                           fused ? kRevTails | kRevPush : kRevTails);
    const int tiles = (b.frame + kRevOut - 1) / kRevOut;
    if (b.n_plain > 0)
        hipLaunchKernelGGL(reverb_batch_conv_kernel<false>, dim3(tiles, 2, b.n_plain), dim3(kBlock), 0, s, b.items, b.plain, b.ir_size,
                           b.cur, b.frame, b.out);
    if (b.n_fade > 0)
        hipLaunchKernelGGL(reverb_batch_conv_kernel<true>, dim3(tiles, 2, b.n_fade), dim3(kBlock), 0, s, b.items, b.fade, b.ir_size,
                           b.cur, b.frame, b.out);
    if (!fused && b.n_plain + b.n_fade > 0)
        hipLaunchKernelGGL(reverb_batch_prepare_kernel, rows, dim3(tb), 0, s, b.items, b.in, b.cur, b.out, b.frame, b.literal_tail, kRevPush);
    if (b.pitems) launch_reverb_part(b.pitems, b.part, b.part_rows, b.ear_rows, b.count, b.literal_tail, b.in, b.out, s);
    if (b.mix) launch_callback_mix(b.out, b.count, 2 * b.frame, b.mix, s);
}

}  // namespace fs
