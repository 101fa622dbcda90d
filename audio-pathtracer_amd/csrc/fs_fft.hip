// fs_fft.hip — frequency-domain material filter for gfx950 (row f4).
//
// Replaces UMaterialAcousticProcessor::ApplyMaterialFD
// (Plugins/FrequenSee/Source/FrequenSee/Private/MaterialAcousticProcessor.cpp:8-107): one forward FFT of the
// zero-padded block, per-bin specular / diffuse / transmitted gains (:51-72), three inverse FFTs, scale 1/N.
//
// Design: a radix-2 complex FFT pair that never runs a bit-reversal pass.
//   forward  = decimation in frequency, natural order in  -> bit-reversed order out;
//   the gains are applied in bit-reversed order (the bin of position p is brev(p));
//   inverse  = decimation in time, bit-reversed order in -> natural order out.
// Stages whose butterfly span fits a 2048-point chunk run inside LDS (one workgroup per chunk, 11 stages per
// launch); wider spans are one global pass each.  For the plugin's block sizes (N <= 65536) that is
// 1 + 5 + 1 launches forward and the same inverse, the three inverse transforms batched over blockIdx.y.
// Twiddles come from a table computed in double precision on the host (W[k] = exp(-2 pi i k / N), k < N/2).
// The inverse passes also build the band carriers of FS_FLAG_SPECTRAL_IR (launch_build_carriers, at the end of the file).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs_internal.hpp"

namespace fs {
namespace {

constexpr int kFftBlock = 256;

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}
__device__ __forceinline__ float2 cmul_conj(float2 a, float2 w) {   // a * conj(w)
    return make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y);
}

// MAP.cpp:51-72 — the gain of output `which` (0 specular, 1 diffuse, 2 transmitted) at one bin
__device__ __forceinline__ float material_gain(int which, float alpha, float tau, float sigma) {
    const float refl = 1.0f - alpha;
    if (refl + tau > 1.0f) tau = 1.0f - refl;   // energy conservation
    return which == 0 ? refl * (1.0f - sigma) : (which == 1 ? refl * sigma : tau);
}

// ---- forward, spans >= one chunk: one butterfly per thread ----
// in_real != nullptr: first pass, reads the zero-padded real block instead of x
__global__ __launch_bounds__(kFftBlock) void fft_dif_global(const float* __restrict__ in_real, int L,
                                                            float2* __restrict__ x, const float2* __restrict__ W,
                                                            int n, int ls) {
    const uint32_t t = blockIdx.x * kFftBlock + threadIdx.x;
    const uint32_t half = 1u << (n - 1);
    if (t >= half) return;
    const uint32_t s = 1u << ls;
    const uint32_t j = t & (s - 1u);
    const uint32_t i0 = ((t >> ls) << (ls + 1)) + j, i1 = i0 + s;
    float2 a, b;
    if (in_real) {
        a = make_float2(i0 < (uint32_t)L ? in_real[i0] : 0.0f, 0.0f);
        b = make_float2(i1 < (uint32_t)L ? in_real[i1] : 0.0f, 0.0f);
    } else {
        a = x[i0]; b = x[i1];
    }
    x[i0] = cadd(a, b);
    x[i1] = cmul(csub(a, b), W[(size_t)j << (n - 1 - ls)]);
}

// ---- forward, the last c stages inside LDS on chunks of 2^c points ----
__global__ __launch_bounds__(kFftBlock) void fft_dif_local(const float* __restrict__ in_real, int L,
                                                           float2* __restrict__ x, const float2* __restrict__ W,
                                                           int n, int c) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const uint32_t C = 1u << c;
    const uint32_t base = blockIdx.x << c;
    for (uint32_t i = threadIdx.x; i < C; i += kFftBlock) {
        const uint32_t p = base + i;
        sh[i] = in_real ? make_float2(p < (uint32_t)L ? in_real[p] : 0.0f, 0.0f) : x[p];
    }
    for (int ls = c - 1; ls >= 0; --ls) {
        __syncthreads();
        const uint32_t s = 1u << ls;
        for (uint32_t t = threadIdx.x; t < (C >> 1); t += kFftBlock) {
            const uint32_t j = t & (s - 1u);
            const uint32_t i0 = ((t >> ls) << (ls + 1)) + j, i1 = i0 + s;
            const float2 a = sh[i0], b = sh[i1];
            sh[i0] = cadd(a, b);
            sh[i1] = cmul(csub(a, b), W[(size_t)j << (n - 1 - ls)]);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < C; i += kFftBlock) x[base + i] = sh[i];
}

// ---- inverse, first c stages inside LDS; applies the gains while loading.  blockIdx.y = output ----
// c == n: the whole transform fits one chunk and the kernel writes the scaled real block itself.
__global__ __launch_bounds__(kFftBlock) void fft_dit_local(const float2* __restrict__ X, float2* __restrict__ y,
                                                           const float* __restrict__ absorption,
                                                           const float* __restrict__ transmission,
                                                           const float* __restrict__ scattering,
                                                           const float2* __restrict__ W, int n, int c, int L,
                                                           float* __restrict__ out, float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 sh[];
    const int which = blockIdx.y;
    const uint32_t C = 1u << c;
    const uint32_t N = 1u << n;
    const uint32_t base = blockIdx.x << c;
    for (uint32_t i = threadIdx.x; i < C; i += kFftBlock) {
        const uint32_t p = base + i;
        const uint32_t k = n ? (__brev(p) >> (32 - n)) : 0u;   // the bin stored at position p
        const uint32_t kk = k <= (N >> 1) ? k : N - k;          // real input: X[N-k] = conj(X[k]), same gain
        const float g = material_gain(which, absorption[kk], transmission[kk], scattering[kk]);
        const float2 v = X[p];
        sh[i] = make_float2(v.x * g, v.y * g);
    }
    for (int ls = 0; ls < c; ++ls) {
        __syncthreads();
        const uint32_t s = 1u << ls;
        for (uint32_t t = threadIdx.x; t < (C >> 1); t += kFftBlock) {
            const uint32_t j = t & (s - 1u);
            const uint32_t i0 = ((t >> ls) << (ls + 1)) + j, i1 = i0 + s;
            const float2 a = sh[i0];
            const float2 b = cmul_conj(sh[i1], W[(size_t)j << (n - 1 - ls)]);
            sh[i0] = cadd(a, b);
            sh[i1] = csub(a, b);
        }
    }
    __syncthreads();
    if (c == n) {
        for (uint32_t i = threadIdx.x; i < C && i < (uint32_t)L; i += kFftBlock)
            out[(size_t)which * L + i] = sh[i].x * scale;
    } else {
        for (uint32_t i = threadIdx.x; i < C; i += kFftBlock) y[(size_t)which * N + base + i] = sh[i];
    }
}

// ---- inverse, spans >= one chunk; the last stage (ls == n-1) writes the scaled real block ----
__global__ __launch_bounds__(kFftBlock) void fft_dit_global(float2* __restrict__ y, const float2* __restrict__ W, int n,
                                                            int ls, int L, float* __restrict__ out, float scale) {
    const uint32_t t = blockIdx.x * kFftBlock + threadIdx.x;
    const uint32_t half = 1u << (n - 1);
    if (t >= half) return;
    const int which = blockIdx.y;
    float2* yy = y + ((size_t)which << n);
    const uint32_t s = 1u << ls;
    const uint32_t j = t & (s - 1u);
    const uint32_t i0 = ((t >> ls) << (ls + 1)) + j, i1 = i0 + s;
    const float2 a = yy[i0];
    const float2 b = cmul_conj(yy[i1], W[(size_t)j << (n - 1 - ls)]);
    if (ls == n - 1) {
        if (i0 < (uint32_t)L) out[(size_t)which * L + i0] = (a.x + b.x) * scale;
        if (i1 < (uint32_t)L) out[(size_t)which * L + i1] = (a.x - b.x) * scale;
    } else {
        yy[i0] = cadd(a, b);
        yy[i1] = csub(a, b);
    }
}

// ---- FS_FLAG_SPECTRAL_IR: the band carriers (launch_build_carriers).  blockIdx.y = band ----
// splitmix64 (Steele, Lea, Flood 2014): the bin's phase from its index alone
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the band's one-sided spectrum in bit-reversed order: position p holds bin k = brev(p); bins [lo_b, lo_{b+1}) of the band
// get exp(i phi_k), phi_k = 2 pi (splitmix64(seed + k) >> 40) 2^-24 (cos / sin in double), every other bin 0.  seed = kCarrierSeed +
// (c << 32) for channel c of the soundfield reverb, c = 0 for the spectral IR: channel 0 has its phases, and the streams seed + k
// (k < 2^24) of two channels never meet
__global__ __launch_bounds__(kFftBlock) void carrier_spectrum(float2* __restrict__ X, int n, int c, CarrierBands bands) {
    const uint32_t p = blockIdx.x * kFftBlock + threadIdx.x;
    if (p >= (1u << n)) return;
    const int b = blockIdx.y;
    const uint32_t k = __brev(p) >> (32 - n);
    float2 v = make_float2(0.0f, 0.0f);
    if ((int)k >= bands.lo[b] && (int)k < bands.lo[b + 1]) {
        const uint64_t seed = kCarrierSeed + ((uint64_t)(uint32_t)c << 32);
        const double turns = (double)(uint32_t)(splitmix64(seed + k) >> 40) * 0x1p-24;   // (exact)
        double sn, cs;
        sincospi(2.0 * turns, &sn, &cs);
        v = make_float2((float)cs, (float)sn);
    }
    X[((size_t)b << n) + p] = v;
}
// c_b = r_b sqrt(N / sum_{n<N} r_b^2), in place (the sum in double, one workgroup per band); the row's padding up to ld is zeroed
__global__ __launch_bounds__(kFftBlock) void carrier_normalise(float* __restrict__ c, int N, int ld) {
    __shared__ double s_sum[kFftBlock];
    float* row = c + (size_t)blockIdx.x * ld;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += kFftBlock) acc += (double)row[i] * (double)row[i];
    s_sum[threadIdx.x] = acc;
    for (int w = kFftBlock / 2; w > 0; w >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
    }
    __syncthreads();
    const float g = s_sum[0] > 0.0 ? (float)sqrt((double)N / s_sum[0]) : 0.0f;
    for (int i = threadIdx.x; i < ld; i += kFftBlock) row[i] = i < N ? row[i] * g : 0.0f;
}

// ---- fs_reverb_ears_set: the mid and side carriers (launch_build_ear_carriers).  blockIdx.y = row: [0, B) mid, [B, 2B) side ----
// As carrier_spectrum, with the diffuse-field weight: gamma_k = sin(x_k) / x_k, x_k = 2 pi f_k (2 radius) / c, f_k = k fs / K; the mid
// row gets a_k exp(i phi_k), a_k = sqrt((1 + gamma_k) / 2), the side row b_k exp(i psi_k), b_k = sqrt((1 - gamma_k) / 2), psi_k from
// kEarSideSeed.  Everything in double, each product rounded to float once.
__global__ __launch_bounds__(kFftBlock) void ear_carrier_spectrum(float2* __restrict__ X, int n, int B, CarrierBands bands, double fs,
                                                                  double radius_cm, double speed_cm_s) {
    const uint32_t p = blockIdx.x * kFftBlock + threadIdx.x;
    if (p >= (1u << n)) return;
    const int row = blockIdx.y;
    const bool side = row >= B;
    const int b = side ? row - B : row;
    const uint32_t k = __brev(p) >> (32 - n);
    float2 v = make_float2(0.0f, 0.0f);
    if ((int)k >= bands.lo[b] && (int)k < bands.lo[b + 1]) {
        const double f = (double)k * fs / (double)(1u << n);
        const double x = 2.0 * 3.14159265358979323846 * f * (2.0 * radius_cm) / speed_cm_s;
        const double gamma = x == 0.0 ? 1.0 : sin(x) / x;
        const double wgt = side ? sqrt((1.0 - gamma) / 2.0) : sqrt((1.0 + gamma) / 2.0);
        const double turns = (double)(uint32_t)(splitmix64((side ? kEarSideSeed : kCarrierSeed) + k) >> 40) * 0x1p-24;   // (exact)
        double sn, cs;
        sincospi(2.0 * turns, &sn, &cs);
        v = make_float2((float)(wgt * cs), (float)(wgt * sn));
    }
    X[((size_t)row << n) + p] = v;
}
// One scale for the band's two rows: g_b = sqrt(N / sum_{n<N} (r^M_b[n]^2 + r^S_b[n]^2)), the sum in double, one workgroup per band;
// both rows in place, their padding up to ld zeroed.  c: [2][B][ld].
__global__ __launch_bounds__(kFftBlock) void ear_carrier_normalise(float* __restrict__ c, int B, int N, int ld) {
    __shared__ double s_sum[kFftBlock];
    float* mid = c + (size_t)blockIdx.x * ld;
    float* sid = c + ((size_t)B + blockIdx.x) * ld;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += kFftBlock) acc += (double)mid[i] * (double)mid[i] + (double)sid[i] * (double)sid[i];
    s_sum[threadIdx.x] = acc;
    for (int w = kFftBlock / 2; w > 0; w >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
    }
    __syncthreads();
    const float g = s_sum[0] > 0.0 ? (float)sqrt((double)N / s_sum[0]) : 0.0f;
    for (int i = threadIdx.x; i < ld; i += kFftBlock) {
        mid[i] = i < N ? mid[i] * g : 0.0f;
        sid[i] = i < N ? sid[i] * g : 0.0f;
    }
}

// The real part of the inverse transform of `rows` spectra X [rows][K] (K = 2^n, bit-reversed order) through the material filter's
// own inverse passes, unscaled: gains all 1 (alpha = sigma = 0 from `zeros`; which = 0 per row for the LDS pass, whose input is one
// array; the global passes batched over the rows on blockIdx.y).  y: [rows][K] work buffer; out: [rows][ld], the first ld samples.
void inverse_rows(int rows, int n, int ld, const float2* X, float2* y, const float2* W, const float* zeros, float* out, hipStream_t s) {
    const int K = 1 << n;
    const int c = n < kFftChunkLog ? n : kFftChunkLog;
    const size_t lds = sizeof(float2) << c;
    for (int r = 0; r < rows; ++r)
        hipLaunchKernelGGL(fft_dit_local, dim3(1u << (n - c), 1), dim3(kFftBlock), lds, s, X + ((size_t)r << n), y + ((size_t)r << n),
                           zeros, zeros, zeros, W, n, c, ld, out + (size_t)r * ld, 1.0f);
    const unsigned half_blocks = (unsigned)(((K >> 1) + kFftBlock - 1) / kFftBlock);
    for (int ls = c; ls < n; ++ls)
        hipLaunchKernelGGL(fft_dit_global, dim3(half_blocks, (unsigned)rows), dim3(kFftBlock), 0, s, y, W, n, ls, ld, out, 1.0f);
}
unsigned spectrum_blocks(int n) { return (unsigned)(((1 << n) + kFftBlock - 1) / kFftBlock); }

}  // namespace

// x: [N] complex work buffer, y: [3][N], W: [max(N/2,1)] twiddles, resp: absorption | transmission | scattering
// ([3][N/2+1]), out: [3][L] (specular | diffuse | transmitted).  n = log2 N.
void launch_apply_material_fd(const float* in, int L, int n, float2* x, float2* y, const float2* W, const float* resp,
                              float* out, hipStream_t s) {
    const int N = 1 << n;
    const int bins = N / 2 + 1;
    const int c = n < kFftChunkLog ? n : kFftChunkLog;
    const size_t lds = sizeof(float2) << c;
    const unsigned half_blocks = n ? (unsigned)(((N >> 1) + kFftBlock - 1) / kFftBlock) : 0u;
    const float scale = 1.0f / (float)N;   // MAP.cpp:88
    // forward
    for (int ls = n - 1; ls >= c; --ls)
        hipLaunchKernelGGL(fft_dif_global, dim3(half_blocks), dim3(kFftBlock), 0, s, ls == n - 1 ? in : nullptr, L, x, W,
                           n, ls);
    hipLaunchKernelGGL(fft_dif_local, dim3(1u << (n - c)), dim3(kFftBlock), lds, s, c == n ? in : nullptr, L, x, W, n, c);
    // gains + inverse, three outputs at once
    hipLaunchKernelGGL(fft_dit_local, dim3(1u << (n - c), 3), dim3(kFftBlock), lds, s, x, y, resp, resp + bins,
                       resp + 2 * bins, W, n, c, L, out, scale);
    for (int ls = c; ls < n; ++ls)
        hipLaunchKernelGGL(fft_dit_global, dim3(half_blocks, 3), dim3(kFftBlock), 0, s, y, W, n, ls, L, out, scale);
}

}  // namespace fs

namespace fs {

// The band carriers of FS_FLAG_SPECTRAL_IR: r_b[t] = sum_{k in band b} cos(2 pi k t / K + phi_k), t < N, K = 2^n >= N — the real
// part of the inverse DFT of the band's unit-magnitude random-phase one-sided spectrum (inverse_rows) — then scaled to a mean square
// of 1 over the IR.  X, y: [B][K] complex work buffers, W: [max(K/2,1)] twiddles (exp(-2 pi i k / K), double precision on the host),
// zeros: [K/2 + 1], out: [B][ld] (ld >= N, ld <= K or the row is zero-padded).
void launch_build_carriers(int B, int n, int N, int ld, const CarrierBands& bands, float2* X, float2* y, const float2* W,
                           const float* zeros, float* out, hipStream_t s) {
    hipLaunchKernelGGL(carrier_spectrum, dim3(spectrum_blocks(n), (unsigned)B), dim3(kFftBlock), 0, s, X, n, 0, bands);
    inverse_rows(B, n, ld, X, y, W, zeros, out, s);
    hipLaunchKernelGGL(carrier_normalise, dim3((unsigned)B), dim3(kFftBlock), 0, s, out, N, ld);
}

// The two-ear reverb's carriers (fs_reverb_ears_set; definition: DESIGN.md section 8, "Two-ear late reverb"): 2B rows through the same
// passes — rows [0, B) the mid carriers cm_b, rows [B, 2B) the side carriers cs_b — and one scale per band over its two rows.
// X, y: [2B][K] complex work buffers; W, zeros as above; out: [2][B][ld].
void launch_build_ear_carriers(int B, int n, int N, int ld, const CarrierBands& bands, double fs, double radius_cm, double speed_cm_s,
                               float2* X, float2* y, const float2* W, const float* zeros, float* out, hipStream_t s) {
    hipLaunchKernelGGL(ear_carrier_spectrum, dim3(spectrum_blocks(n), (unsigned)(2 * B)), dim3(kFftBlock), 0, s, X, n, B, bands, fs, radius_cm,
                       speed_cm_s);
    inverse_rows(2 * B, n, ld, X, y, W, zeros, out, s);
    hipLaunchKernelGGL(ear_carrier_normalise, dim3((unsigned)B), dim3(kFftBlock), 0, s, out, B, N, ld);
}

// The soundfield reverb's carriers (fs_reverb_soundfield_set; definition: DESIGN.md section 8, "Soundfield late reverb"): the band
// carriers' passes once per channel, with the channel's phases, through one pair of [B][K] work buffers (the stream orders the
// channels); then every one of the C B rows gets the scale of a row of its own, g_{c,b} = sqrt(N / sum r_{c,b}^2).  out: [C][B][ld].
void launch_build_soundfield_carriers(int C, int B, int n, int N, int ld, const CarrierBands& bands, float2* X, float2* y, const float2* W,
                                      const float* zeros, float* out, hipStream_t s) {
    for (int ch = 0; ch < C; ++ch) {
        hipLaunchKernelGGL(carrier_spectrum, dim3(spectrum_blocks(n), (unsigned)B), dim3(kFftBlock), 0, s, X, n, ch, bands);
        inverse_rows(B, n, ld, X, y, W, zeros, out + (size_t)ch * (size_t)B * (size_t)ld, s);
    }
    hipLaunchKernelGGL(carrier_normalise, dim3((unsigned)(C * B)), dim3(kFftBlock), 0, s, out, N, ld);
}

}  // namespace fs
