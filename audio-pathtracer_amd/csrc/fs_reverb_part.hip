// fs_reverb_part.hip — row f2, the reverb callback's PARTITIONED engine (fs_reverb_set_engine): a uniformly partitioned
// overlap-save convolution with a frequency-domain delay line, beside the direct form of fs_reverb.hip.
//
// With frame F, N = the smallest power of two >= 2F and K = ceil(ir_size / F):
//   H_p = FFT_N(h[pF .. pF + F) zero-padded), p < K                      reverb_part_take_kernel (only when a newer IR is taken)
//   X_t = FFT_N(w_L + i w_R), w = the last N samples ending in this block  reverb_part_forward_kernel -> a ring of K spectra
//   Y   = sum_{p < K} H_p X_{t-p}                                         reverb_product_kernel
//   y   = IFFT_N(Y); out = the last F of y, real part left, imaginary part right   reverb_part_inverse_kernel
// The IR is real and mono, so one complex transform carries both channels.  The cost of a callback is K N complex MACs and
// three N-point transforms (0.1 M MACs at F = 1024 and 48 000 taps; the direct form needs 98 M), and the history is one window
// whatever the IR length.
//
// The transforms are the radix-2 pair of fs_fft.hip, whole inside LDS (N <= 4096: 32 KB of float2, one workgroup each): forward =
// decimation in frequency, natural order in, bit-reversed order out; inverse = decimation in time, bit-reversed in, natural
// out.  H, X and Y all live in bit-reversed order and the product is pointwise, so no bit-reversal pass exists.  Twiddles come
// from the host's double-precision table (W[k] = exp(-2 pi i k / N), k < N / 2, cached per N in the context).
//
// Every kernel finds its row through a table of ReverbPartItem (fs_internal.hpp), the rows of a call side by side in the grid;
// nothing a row computes depends on the other rows, so a source gets the same bits alone or in any batch.  The file is built
// with -ffp-contract=off: what is fused is written as fmaf.
//
// ONE engine, three kinds of row.  They share the delay line, the product's scaffold (reverb_product_kernel: tiling, slot walk,
// order of sums), the inverse with its fade (reverb_part_inverse_kernel) and the fold of a cut-short fade (fold_cut_short); a kind
// says how many products a row keeps, what one partition adds to each and how its state block is laid out (PlainRow, EarRow, BusRow):
//   plain   one spectrum set per IR copy, from the mono IR; a stereo window (left + i right)         reverb_part_take_kernel
//   ears    (fs_reverb_set_ears) two sets, M_p and S_p, from the band rows and the ear carriers; the product adds the mirrored
//           bin's term; window, delay line and inverse are the plain row's                          reverb_ears_take_kernel
//   bus     (fs_reverb_set_soundfield) P = ceil(C / 2) sets, complex IRs that each carry two channels of the ambisonic bus; a
//           mono window (reverb_soundfield_forward_kernel), P products and one inverse per pair     reverb_soundfield_take_kernel
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs_internal.hpp"

namespace fs {
namespace {

constexpr int kPartBlock = 256;
constexpr int kMacBins = 64;                        // bins per multiply-accumulate workgroup: one wavefront wide
constexpr int kMacWaves = kPartBlock / kMacBins;    // its wavefronts share the partitions: wave w takes p = w, w + 4, ...
constexpr uint32_t kEarsMaxFrame = 2048;            // the engine's largest frame (fs_reverb_init), N <= 2 * kEarsMaxFrame

__device__ __forceinline__ float2 padd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 psub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 pmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 pmul_conj(float2 a, float2 w) { return make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y); }
// acc + h x, each component two fused steps in a fixed order
__device__ __forceinline__ float2 pmac(float2 acc, float2 h, float2 x) {
    return make_float2(fmaf(h.x, x.x, fmaf(-h.y, x.y, acc.x)), fmaf(h.x, x.y, fmaf(h.y, x.x, acc.y)));
}

// sh[0 .. 2^n): natural order -> the spectrum in bit-reversed order.  Every thread of the workgroup calls it; sh is complete
// before (the caller's stores need no barrier of their own) and after.
__device__ __forceinline__ void lds_fft_dif(float2* sh, const float2* __restrict__ W, int n) {
    const uint32_t half = 1u << (n - 1);
    for (int ls = n - 1; ls >= 0; --ls) {
        __syncthreads();
        const uint32_t s = 1u << ls;
        for (uint32_t t = threadIdx.x; t < half; t += kPartBlock) {
            const uint32_t j = t & (s - 1u);
            const uint32_t i0 = ((t >> ls) << (ls + 1)) + j, i1 = i0 + s;
            const float2 a = sh[i0], b = sh[i1];
            sh[i0] = padd(a, b);
            sh[i1] = pmul(psub(a, b), W[(size_t)j << (n - 1 - ls)]);
        }
    }
    __syncthreads();
}
// sh[0 .. 2^n): a spectrum in bit-reversed order -> N times its inverse transform in natural order
__device__ __forceinline__ void lds_fft_dit(float2* sh, const float2* __restrict__ W, int n) {
    const uint32_t half = 1u << (n - 1);
    for (int ls = 0; ls < n; ++ls) {
        __syncthreads();
        const uint32_t s = 1u << ls;
        for (uint32_t t = threadIdx.x; t < half; t += kPartBlock) {
            const uint32_t j = t & (s - 1u);
            const uint32_t i0 = ((t >> ls) << (ls + 1)) + j, i1 = i0 + s;
            const float2 a = sh[i0];
            const float2 b = pmul_conj(sh[i1], W[(size_t)j << (n - 1 - ls)]);
            sh[i0] = padd(a, b);
            sh[i1] = psub(a, b);
        }
    }
    __syncthreads();
}

// The fold of a fade that is cut short, on partition p of `sets` spectrum sets (h_from, h_to: the partition in the first set, `set`
// float2 from one set to the next): H_from[p] := (1 - a) H_from[p] + a H_to[p], a = p0 / L > 0 — exact on the spectra, the transform
// is linear.  Every thread of the workgroup calls it.
__device__ __forceinline__ void fold_cut_short(float2* __restrict__ h_from, const float2* __restrict__ h_to, size_t set, int sets, float a,
                                               uint32_t N) {
    for (int q = 0; q < sets; ++q)
        for (uint32_t i = threadIdx.x; i < N; i += kPartBlock) {
            const float2 f = h_from[q * set + i], t = h_to[q * set + i];
            h_from[q * set + i] = make_float2((1.0f - a) * f.x + a * t.x, (1.0f - a) * f.y + a * t.y);
        }
}

// The rows of `take` get a newer IR: workgroup (p, k) owns partition p of row take[k].  First the fold (when take_a > 0), then
// H_to[p] := FFT_N(ir[pF .. pF + F) zero-padded).
__global__ __launch_bounds__(kPartBlock) void reverb_part_take_kernel(const ReverbPartItem* __restrict__ items, const int* __restrict__ take,
                                                                      const float2* __restrict__ W, int n, int frame, int ir_size) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const ReverbPartItem it = items[take[blockIdx.y]];
    const uint32_t N = 1u << n;
    const uint32_t p = blockIdx.x;
    float2* __restrict__ h_to = it.take_to + (size_t)p * N;
    if (it.take_a > 0.0f) fold_cut_short(it.take_from + (size_t)p * N, h_to, 0, 1, it.take_a, N);
    const float* __restrict__ ir = it.take_ir;
    const uint32_t k0 = p * (uint32_t)frame;
    for (uint32_t i = threadIdx.x; i < N; i += kPartBlock)
        sh[i] = make_float2(i < (uint32_t)frame && k0 + i < (uint32_t)ir_size ? ir[k0 + i] : 0.0f, 0.0f);
    lds_fft_dif(sh, W, n);
    for (uint32_t i = threadIdx.x; i < N; i += kPartBlock) h_to[i] = sh[i];
}

// Row r = blockIdx.x (left at once unless it is a convolved row of this engine): the transform of its window.  The window's
// first N - F samples come from the history ring (N complex samples, left + i right, head = the sample this block starts at),
// the last F are this block.  blockIdx.y == 0: the true block, which also enters the history; its transform enters the spectrum
// ring at `slot`.  blockIdx.y == 1 (FS_REVERB_LITERAL_TAIL only): the block as RVB.cpp:147-148 reads it — the interleaved
// buffer's first F floats in both channels — into the row's x_now, which this callback's product reads in place of the slot.
// The history positions the first workgroup writes, [head, head + F), are not among those either reads, [head + F, head + N).
__global__ __launch_bounds__(kPartBlock) void reverb_part_forward_kernel(const ReverbPartItem* __restrict__ items, const float* __restrict__ in_all,
                                                                         const float2* __restrict__ W, int n, int frame) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const int r = blockIdx.x;
    const ReverbPartItem it = items[r];
    if (!it.active) return;
    const uint32_t N = 1u << n;
    const bool literal = blockIdx.y != 0;
    const float* __restrict__ in = in_all + (size_t)r * 2 * (size_t)frame;
    float2* __restrict__ hist = part_hist(it.state);
    const uint32_t old = N - (uint32_t)frame;
    for (uint32_t j = threadIdx.x; j < N; j += kPartBlock) {
        float2 v;
        if (j < old) {
            v = hist[(it.head + (uint32_t)frame + j) & (N - 1u)];
        } else {
            const uint32_t i = j - old;
            if (literal) {
                v = make_float2(in[i], in[i]);
            } else {
                v = make_float2(in[2 * i], in[2 * i + 1]);
                hist[(it.head + i) & (N - 1u)] = v;
            }
        }
        sh[j] = v;
    }
    lds_fft_dif(sh, W, n);
    float2* __restrict__ dst = literal ? part_xnow(it.state, n) : part_xring(it.state, n, true, 1) + ((size_t)it.slot << n);
    for (uint32_t j = threadIdx.x; j < N; j += kPartBlock) dst[j] = sh[j];
}

// acc + s conj(x), each component two fused steps in a fixed order
__device__ __forceinline__ float2 pmac_conj(float2 acc, float2 s, float2 x) {
    return make_float2(fmaf(s.x, x.x, fmaf(s.y, x.y, acc.x)), fmaf(s.y, x.x, fmaf(-s.x, x.y, acc.y)));
}

// The three kinds of row, as the product sees them: kAcc products per IR copy, kStereo (the state block's layout, and whether a
// literal tail exists), kMirror (whether step reads the window's mirrored bin too), the unroll of the partition loop, and step — what
// partition p adds to one product: H the bin in partition p of the product's first spectrum set, `set` float2 from a set to the
// next, x the window spectrum's bin and xm its mirror's.
struct PlainRow {   // acc += H_p X
    static constexpr int kAcc = 1, kUnroll = 4;
    static constexpr bool kStereo = true, kMirror = false;
    static __device__ __forceinline__ float2 step(float2 acc, const float2* __restrict__ H, size_t set, float2 x, float2 xm) {
        return pmac(acc, H[0], x);
    }
};
// Both channels through the one packed transform: Y[k] = M_p[k] X[k] + S_p[k] conj(X[(N - k) mod N]).  Position j of the bit-reversed
// storage holds bin brev(j); the bin N - brev(j) (mod N) lives at jm = brev((N - brev(j)) mod N).  The mirrors of a 64-aligned block
// of positions are one 64-aligned block (read in descending order, except block 0's), so a wavefront's mirrored load is 512
// contiguous bytes too.
struct EarRow {     // acc += M_p X, then acc += S_p conj(X_mirror)
    static constexpr int kAcc = 1, kUnroll = 4;
    static constexpr bool kStereo = true, kMirror = true;
    static __device__ __forceinline__ float2 step(float2 acc, const float2* __restrict__ H, size_t set, float2 x, float2 xm) {
        return pmac_conj(pmac(acc, H[0], x), H[set], xm);
    }
};
// P spectrum streams against the one X: each X_{t-p}[b] is loaded once and multiplied into the P (FADE: 2 P) products of the pairs,
// which stay in registers because P is a template argument
template <int P>
struct BusRow : PlainRow {
    static constexpr int kAcc = P, kUnroll = 2;
    static constexpr bool kStereo = false;
};

// The product of row list[blockIdx.y] over the delay line: Y_q[b] = sum_p H_{q,p}[b] X_{t-p}[b] (Row::step), X_{t-p} = spectrum ring
// slot (slot - p) mod K (p = 0 of a stereo row: x_now in a literal-tail callback).  A workgroup owns 64 adjacent bins, so every load
// of a wavefront is 512 contiguous bytes; its four wavefronts take p = w, w + 4, ... in ascending order and their sums meet in LDS
// as ((s0 + s1) + s2) + s3 — an order fixed by K alone.  FADE: the same X against H_from and H_to, two sums per product.
// Y: [2][kAcc][N], the products with H, then (FADE) with H_to.
template <class Row, bool FADE>
__global__ __launch_bounds__(kPartBlock) void reverb_product_kernel(const ReverbPartItem* __restrict__ items, const int* __restrict__ list,
                                                                    int n, int K, int literal) {
    constexpr int A = Row::kAcc;
    __shared__ float2 s_sum[FADE ? 2 : 1][A][kMacWaves][kMacBins];
    const ReverbPartItem it = items[list[blockIdx.y]];
    const uint32_t N = 1u << n;
    const uint32_t lane = threadIdx.x & (kMacBins - 1), w = threadIdx.x / kMacBins;
    const uint32_t b = blockIdx.x * kMacBins + lane;
    const bool live = b < N;   // (N = 32: half a wavefront)
    const uint32_t bm = __brev((N - (__brev(b) >> (32 - n))) & (N - 1u)) >> (32 - n);   // (live: < N; the ear row's)
    const size_t set = (size_t)K << n;
    const float2* __restrict__ H = it.h;
    const float2* __restrict__ H_to = it.h_to;
    const float2* __restrict__ xring = part_xring(it.state, n, Row::kStereo, A);
    const float2* __restrict__ xnow = part_xnow(it.state, n);
    float2 acc[A], acc_to[A];
#pragma unroll
    for (int q = 0; q < A; ++q) acc[q] = acc_to[q] = make_float2(0.0f, 0.0f);
    if (live) {
#pragma unroll Row::kUnroll
        for (int p = (int)w; p < K; p += kMacWaves) {
            int sp = it.slot - p;
            sp += sp < 0 ? K : 0;
            const bool now = Row::kStereo && p == 0 && literal;
            const size_t slot = (size_t)sp << n;
            float2 x, xm;
            if (Row::kMirror) {   // two bins of one spectrum: choose the spectrum
                const float2* __restrict__ X = now ? xnow : xring + slot;
                x = X[b], xm = X[bm];
            } else {              // one bin: choose the value (a branch round one load keeps fewer addresses live than a select of them)
                x = xm = now ? xnow[b] : xring[slot + b];
            }
            const size_t at = ((size_t)p << n) + b;
#pragma unroll
            for (int q = 0; q < A; ++q) {
                acc[q] = Row::step(acc[q], H + (q * set + at), set, x, xm);
                if (FADE) acc_to[q] = Row::step(acc_to[q], H_to + (q * set + at), set, x, xm);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < A; ++q) {
        s_sum[0][q][w][lane] = acc[q];
        if (FADE) s_sum[FADE ? 1 : 0][q][w][lane] = acc_to[q];
    }
    __syncthreads();
    if (w == 0 && live) {
        float2* __restrict__ Y = part_y(it.state, n, Row::kStereo);
#pragma unroll
        for (int q = 0; q < A; ++q) {
            float2 v = s_sum[0][q][0][lane];
#pragma unroll
            for (int k = 1; k < kMacWaves; ++k) v = padd(v, s_sum[0][q][k][lane]);
            Y[((size_t)q << n) + b] = v;
            if (FADE) {
                float2 u = s_sum[FADE ? 1 : 0][q][0][lane];
#pragma unroll
                for (int k = 1; k < kMacWaves; ++k) u = padd(u, s_sum[FADE ? 1 : 0][q][k][lane]);
                Y[((size_t)(A + q) << n) + b] = u;
            }
        }
    }
}

// Workgroup (r, q) inverts product q of row r: y = IFFT_N(Y_q) / N, the last F samples, the real part into channel 2q and the
// imaginary part into channel 2q + 1 of the row's [F][C] block.  A fading row (h_to) inverts both sums and mixes per output sample,
// (1 - g) y_from + g y_to, g = (p + 1) / L while p = fade_pos + s < L, else 1 — the direct engine's expression.
// STEREO: one product and C = 2 (left, right), whatever P and C say; rows that are not convolved rows of this engine are left at
// once; the output is clamped (FMath::Clamp RVB.cpp:165-167, MixAlpha = 1).  The bus: P products per row, the last one without a
// partner at odd C, NOT clamped (a bus is summed and decoded before it reaches a converter).
// LDS: the transform [N] and, for the fade, y_from's kept samples [F].
template <bool STEREO>
__global__ __launch_bounds__(kPartBlock) void reverb_part_inverse_kernel(const ReverbPartItem* __restrict__ items, const float2* __restrict__ W,
                                                                         int n, int frame, int P_bus, int C_bus, float* __restrict__ out_all) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const int r = blockIdx.x;
    const int q = STEREO ? 0 : (int)blockIdx.y;
    const int P = STEREO ? 1 : P_bus, C = STEREO ? 2 : C_bus;
    const ReverbPartItem it = items[r];
    if (STEREO && !it.active) return;
    const uint32_t N = 1u << n;
    const float scale = 1.0f / (float)N;   // (a power of two: exact)
    const float2* __restrict__ Y = part_y(it.state, n, STEREO) + ((size_t)q << n);
    const float2* __restrict__ Y_to = Y + ((size_t)P << n);
    float2* keep = sh + N;
    float* __restrict__ out = out_all + (size_t)r * (size_t)C * (size_t)frame;
    const uint32_t old = N - (uint32_t)frame;
    for (uint32_t j = threadIdx.x; j < N; j += kPartBlock) sh[j] = Y[j];
    lds_fft_dit(sh, W, n);
    const bool fade = it.h_to != nullptr;
    if (fade) {
        for (uint32_t s = threadIdx.x; s < (uint32_t)frame; s += kPartBlock) keep[s] = sh[old + s];
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < N; j += kPartBlock) sh[j] = Y_to[j];
        lds_fft_dit(sh, W, n);
    }
    const bool partner = STEREO || 2 * q + 1 < C;
    for (uint32_t s = threadIdx.x; s < (uint32_t)frame; s += kPartBlock) {
        float2 v = sh[old + s];
        v = make_float2(v.x * scale, v.y * scale);
        if (fade) {
            const float2 f = make_float2(keep[s].x * scale, keep[s].y * scale);
            const int p = it.fade_pos + (int)s;
            const float g = p < it.fade_len ? (float)(p + 1) / (float)it.fade_len : 1.0f;
            v = make_float2((1.0f - g) * f.x + g * v.x, (1.0f - g) * f.y + g * v.y);
        }
        if (STEREO) {
            v.x = v.x < -1.0f ? -1.0f : (v.x > 1.0f ? 1.0f : v.x);
            v.y = v.y < -1.0f ? -1.0f : (v.y > 1.0f ? 1.0f : v.y);
        }
        out[(size_t)s * (size_t)C + 2 * q] = v.x;
        if (partner) out[(size_t)s * (size_t)C + 2 * q + 1] = v.y;
    }
}

// ---- sources with ears (fs_reverb_set_ears; definition: DESIGN.md section 8, "Two-ear late reverb") ----
// h_L = m + s, h_R = m - s with m[i] = (1/sqrt(B)) sum_b env_b[i] cm_b[i], s[i] likewise with cs_b: the left channel is convolved
// with h_L and the right with h_R in the one packed transform (EarRow).
//
// (m[i], s[i]): fp32, the bands in ascending order, each product rounded before it is added, the scale last — THE expression of both
// kernels that form them (the take and the copy)
__device__ __forceinline__ float2 ears_mid_side(const float* __restrict__ env, const ReverbEars e, int num_samples, uint32_t i) {
    float m = 0.0f, s = 0.0f;
    const float* __restrict__ cm = e.c + i;
    const float* __restrict__ cs = e.c + (size_t)e.B * (size_t)e.ld + i;
    for (int b = 0; b < e.B; ++b) {
        const float v = env[(size_t)b * (size_t)num_samples + i];
        m = m + v * cm[(size_t)b * (size_t)e.ld];
        s = s + v * cs[(size_t)b * (size_t)e.ld];
    }
    const float g = 1.0f / sqrtf((float)e.B);
    return make_float2(m * g, s * g);
}
// reverb_part_take_kernel for the rows with ears: workgroup (p, k) owns partition p of row take[k], in both spectrum sets of a copy
// ([2][K][N]: M, then S).  The fold of a cut-short fade on both sets, then M_p := FFT_N(m[pF .. pF + F) zero-padded) and S_p likewise
// from the row's B band rows (take_ir) and the carrier set.
__global__ __launch_bounds__(kPartBlock) void reverb_ears_take_kernel(const ReverbPartItem* __restrict__ items, const int* __restrict__ take,
                                                                      const float2* __restrict__ W, int n, int K, int frame, int ir_size,
                                                                      ReverbEars e) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const ReverbPartItem it = items[take[blockIdx.y]];
    const uint32_t N = 1u << n;
    const uint32_t p = blockIdx.x;
    const size_t set = (size_t)K << n;   // from M to S
    float2* __restrict__ h_to = it.take_to + (size_t)p * N;
    if (it.take_a > 0.0f) fold_cut_short(it.take_from + (size_t)p * N, h_to, set, 2, it.take_a, N);
    const uint32_t k0 = p * (uint32_t)frame;
    float side[kEarsMaxFrame / kPartBlock];   // s of the thread's samples of the partition, kept while m is transformed
#pragma unroll
    for (uint32_t q = 0; q < kEarsMaxFrame / kPartBlock; ++q) {
        const uint32_t i = threadIdx.x + q * kPartBlock;
        float2 ms = make_float2(0.0f, 0.0f);
        if (i < (uint32_t)frame && k0 + i < (uint32_t)ir_size) ms = ears_mid_side(it.take_ir, e, ir_size, k0 + i);
        side[q] = ms.y;
        if (i < N) sh[i] = make_float2(ms.x, 0.0f);
    }
    for (uint32_t i = kEarsMaxFrame + threadIdx.x; i < N; i += kPartBlock) sh[i] = make_float2(0.0f, 0.0f);   // (N = 4096: the upper half)
    lds_fft_dif(sh, W, n);
    for (uint32_t i = threadIdx.x; i < N; i += kPartBlock) h_to[i] = sh[i];
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kEarsMaxFrame / kPartBlock; ++q) {
        const uint32_t i = threadIdx.x + q * kPartBlock;
        if (i < N) sh[i] = make_float2(side[q], 0.0f);
    }
    for (uint32_t i = kEarsMaxFrame + threadIdx.x; i < N; i += kPartBlock) sh[i] = make_float2(0.0f, 0.0f);
    lds_fft_dif(sh, W, n);
    for (uint32_t i = threadIdx.x; i < N; i += kPartBlock) h_to[set + i] = sh[i];
}

// fs_reverb_copy_ear_impulse_responses: the ear IRs of one source's band rows, sample by sample
__global__ __launch_bounds__(kPartBlock) void reverb_ears_ir_kernel(const float* __restrict__ bands, ReverbEars e, int num_samples,
                                                                    float* __restrict__ left, float* __restrict__ right) {
    const uint32_t i = blockIdx.x * kPartBlock + threadIdx.x;
    if (i >= (uint32_t)num_samples) return;
    const float2 ms = ears_mid_side(bands, e, num_samples, i);
    left[i] = ms.x + ms.y;
    right[i] = ms.x - ms.y;
}

// ---- soundfield rows (fs_reverb_soundfield_process_batch; definition: DESIGN.md section 8, "Soundfield late reverb") ----
// Channel c of the ACN/SN3D bus is the source's mono downmix convolved with h_c, an IR of its own: the band rows times channel c's
// carriers, weighted for its degree.  The input is real, so channels 2q and 2q + 1 ride in one complex IR: with P = ceil(C / 2)
//   G_{q,p} = FFT_N(h_{2q}[pF .. pF + F) + i h_{2q+1}[pF .. pF + F))        reverb_soundfield_take_kernel
//   X_t     = FFT_N(w + 0 i), w = the mono window                           reverb_soundfield_forward_kernel -> the ring of K spectra
//   Y_q     = sum_p G_{q,p} X_{t-p}, every X read once for all P pairs      reverb_product_kernel<BusRow<P>>
//   IFFT_N(Y_q): the last F samples' real part is channel 2q, the imaginary part channel 2q + 1   reverb_part_inverse_kernel<false>
// (the product of a complex IR spectrum with a real signal's spectrum is the spectrum of the complex convolution: no mirror term).
//
// the degree l of ACN channel c, c < 16
__device__ __forceinline__ int sf_degree(int c) { return c >= 9 ? 3 : (c >= 4 ? 2 : (c >= 1 ? 1 : 0)); }
// h_c[i]: fp32, the bands in ascending order, each product rounded before it is added, the two scales last — THE expression of both
// kernels that form it (the take and the copy)
__device__ __forceinline__ float sf_channel(const float* __restrict__ env, const ReverbSoundfield& e, int num_samples, int c, uint32_t i) {
    float m = 0.0f;
    const float* __restrict__ car = e.c + (size_t)c * (size_t)e.B * (size_t)e.ld + i;
    for (int b = 0; b < e.B; ++b) m = m + env[(size_t)b * (size_t)num_samples + i] * car[(size_t)b * (size_t)e.ld];
    m = m * (1.0f / sqrtf((float)e.B));
    return m * e.w[sf_degree(c)];
}

// reverb_part_take_kernel for the soundfield rows: workgroup (p, k) owns partition p of row take[k] in all P spectrum sets of a copy
// ([P][K][N]).  The fold of a cut-short fade on all sets first, then G_{q,p} for q < P from the row's B band rows (take_ir) and the
// carrier set; at odd C the last pair's imaginary part is zero.
__global__ __launch_bounds__(kPartBlock) void reverb_soundfield_take_kernel(const ReverbPartItem* __restrict__ items, const int* __restrict__ take,
                                                                            const float2* __restrict__ W, int n, int K, int frame,
                                                                            int ir_size, ReverbSoundfield e) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const ReverbPartItem it = items[take[blockIdx.y]];
    const uint32_t N = 1u << n;
    const uint32_t p = blockIdx.x;
    const int P = (e.C + 1) >> 1;
    const size_t set = (size_t)K << n;   // from one pair's spectra to the next's
    float2* __restrict__ h_to = it.take_to + (size_t)p * N;
    if (it.take_a > 0.0f) fold_cut_short(it.take_from + (size_t)p * N, h_to, set, P, it.take_a, N);
    const uint32_t k0 = p * (uint32_t)frame;
    for (int q = 0; q < P; ++q) {
        for (uint32_t i = threadIdx.x; i < N; i += kPartBlock) {
            float2 v = make_float2(0.0f, 0.0f);
            if (i < (uint32_t)frame && k0 + i < (uint32_t)ir_size) {
                v.x = sf_channel(it.take_ir, e, ir_size, 2 * q, k0 + i);
                if (2 * q + 1 < e.C) v.y = sf_channel(it.take_ir, e, ir_size, 2 * q + 1, k0 + i);
            }
            sh[i] = v;
        }
        lds_fft_dif(sh, W, n);
        for (uint32_t i = threadIdx.x; i < N; i += kPartBlock) h_to[q * set + i] = sh[i];
        __syncthreads();   // (sh is read out before the next pair fills it)
    }
}

// reverb_part_forward_kernel for the soundfield rows: row r = blockIdx.x, the transform of its mono window.  The history ring holds
// N floats, d(n) = 0.5f * (in[2n] + in[2n + 1]); the window's first N - F samples come from it, the last F are this block's d, which
// enter it.  The positions written, [head, head + F), are not among those read, [head + F, head + N).
__global__ __launch_bounds__(kPartBlock) void reverb_soundfield_forward_kernel(const ReverbPartItem* __restrict__ items,
                                                                               const float* __restrict__ in_all, const float2* __restrict__ W,
                                                                               int n, int frame, int P) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const int r = blockIdx.x;
    const ReverbPartItem it = items[r];
    const uint32_t N = 1u << n;
    const float* __restrict__ in = in_all + (size_t)r * 2 * (size_t)frame;
    float* __restrict__ hist = (float*)part_hist(it.state);
    const uint32_t old = N - (uint32_t)frame;
    for (uint32_t j = threadIdx.x; j < N; j += kPartBlock) {
        float v;
        if (j < old) {
            v = hist[(it.head + (uint32_t)frame + j) & (N - 1u)];
        } else {
            const uint32_t i = j - old;
            v = 0.5f * (in[2 * i] + in[2 * i + 1]);
            hist[(it.head + i) & (N - 1u)] = v;
        }
        sh[j] = make_float2(v, 0.0f);
    }
    lds_fft_dif(sh, W, n);
    float2* __restrict__ dst = part_xring(it.state, n, false, P) + ((size_t)it.slot << n);
    for (uint32_t j = threadIdx.x; j < N; j += kPartBlock) dst[j] = sh[j];
}

// fs_reverb_copy_soundfield_impulse_responses: channel blockIdx.y's IR of one source's band rows, sample by sample
__global__ __launch_bounds__(kPartBlock) void reverb_soundfield_ir_kernel(const float* __restrict__ bands, ReverbSoundfield e, int num_samples,
                                                                          float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kPartBlock + threadIdx.x;
    if (i >= (uint32_t)num_samples) return;
    const int c = blockIdx.y;
    out[(size_t)c * (size_t)num_samples + i] = sf_channel(bands, e, num_samples, c, i);
}

// the products of one kind's two lists, each launched only when it has rows
template <class Row>
void launch_products(const ReverbPartItem* items, const ReverbShape& p, const ReverbLists& l, int literal_tail, hipStream_t s) {
    const unsigned tiles = ((1u << p.n) + kMacBins - 1) / kMacBins;
    if (l.n_plain > 0)
        hipLaunchKernelGGL((reverb_product_kernel<Row, false>), dim3(tiles, (unsigned)l.n_plain), dim3(kPartBlock), 0, s, items, l.plain, p.n,
                           p.K, literal_tail);
    if (l.n_fade > 0)
        hipLaunchKernelGGL((reverb_product_kernel<Row, true>), dim3(tiles, (unsigned)l.n_fade), dim3(kPartBlock), 0, s, items, l.fade, p.n,
                           p.K, literal_tail);
}

}  // namespace

void launch_reverb_part_take(const ReverbPartItem* items, const int* take, int n_take, const ReverbShape& p, hipStream_t s) {
    hipLaunchKernelGGL(reverb_part_take_kernel, dim3((unsigned)p.K, (unsigned)n_take), dim3(kPartBlock), sizeof(float2) << p.n, s, items,
                       take, p.W, p.n, p.frame, p.ir_size);
}

void launch_reverb_ears_take(const ReverbPartItem* items, const int* take, int n_take, const ReverbShape& p, const ReverbEars& e, hipStream_t s) {
    hipLaunchKernelGGL(reverb_ears_take_kernel, dim3((unsigned)p.K, (unsigned)n_take), dim3(kPartBlock), sizeof(float2) << p.n, s, items,
                       take, p.W, p.n, p.K, p.frame, p.ir_size, e);
}

void launch_reverb_soundfield_take(const ReverbPartItem* items, const int* take, int n_take, const ReverbShape& p, const ReverbSoundfield& e,
                                   hipStream_t s) {
    hipLaunchKernelGGL(reverb_soundfield_take_kernel, dim3((unsigned)p.K, (unsigned)n_take), dim3(kPartBlock), sizeof(float2) << p.n, s,
                       items, take, p.W, p.n, p.K, p.frame, p.ir_size, e);
}

void launch_reverb_ears_ir(const float* bands, const ReverbEars& e, int n, float* left, float* right, hipStream_t s) {
    hipLaunchKernelGGL(reverb_ears_ir_kernel, dim3((unsigned)((n + kPartBlock - 1) / kPartBlock)), dim3(kPartBlock), 0, s, bands, e, n, left,
                       right);
}

void launch_reverb_soundfield_ir(const float* bands, const ReverbSoundfield& e, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(reverb_soundfield_ir_kernel, dim3((unsigned)((n + kPartBlock - 1) / kPartBlock), (unsigned)e.C), dim3(kPartBlock), 0, s,
                       bands, e, n, out);
}

void launch_reverb_part(const ReverbPartItem* items, const ReverbShape& p, const ReverbLists& rows, const ReverbLists& ears, int count,
                        int literal_tail, const float* in, float* out, hipStream_t s) {
    const size_t lds = sizeof(float2) << p.n;
    hipLaunchKernelGGL(reverb_part_forward_kernel, dim3((unsigned)count, literal_tail ? 2u : 1u), dim3(kPartBlock), lds, s, items, in, p.W,
                       p.n, p.frame);
    launch_products<PlainRow>(items, p, rows, literal_tail, s);
    launch_products<EarRow>(items, p, ears, literal_tail, s);
    hipLaunchKernelGGL(reverb_part_inverse_kernel<true>, dim3((unsigned)count), dim3(kPartBlock), lds + sizeof(float2) * (size_t)p.frame, s,
                       items, p.W, p.n, p.frame, 1, 2, out);
}

void launch_reverb_soundfield(const ReverbPartItem* items, const ReverbShape& p, const ReverbLists& rows, const ReverbSoundfield& e, int count,
                              const float* in, float* out, float* mix, hipStream_t s) {
    const size_t lds = sizeof(float2) << p.n;
    const int P = (e.C + 1) / 2;
    hipLaunchKernelGGL(reverb_soundfield_forward_kernel, dim3((unsigned)count), dim3(kPartBlock), lds, s, items, in, p.W, p.n, p.frame, P);
    switch (P) {   // (C = 1, 4, 9, 16)
        case 1: launch_products<BusRow<1>>(items, p, rows, 0, s); break;
        case 2: launch_products<BusRow<2>>(items, p, rows, 0, s); break;
        case 5: launch_products<BusRow<5>>(items, p, rows, 0, s); break;
        default: launch_products<BusRow<8>>(items, p, rows, 0, s); break;
    }
    hipLaunchKernelGGL(reverb_part_inverse_kernel<false>, dim3((unsigned)count, (unsigned)P), dim3(kPartBlock),
                       lds + sizeof(float2) * (size_t)p.frame, s, items, p.W, p.n, p.frame, P, e.C, out);
    if (mix) launch_callback_mix(out, count, p.frame * e.C, mix, s);
}

}  // namespace fs
