// fs_dev_recon.hpp — ReconstructImpulseResponse on the device, the spectral channel row, the zero-block votes of the
// host ring slots and the publish of a launch's host slots.
#pragma once
#include "fs_dev_common.hpp"

namespace fs {
namespace {

// ReconstructImpulseResponse (FSAC.cpp:320-380) for one row (band, or row B = the band mean = the channel view) and one block
// of kBlock chunks of kChunk samples; s_amp: [nb] floats of LDS.  Shared by reconstruct_kernel (tail stream) and the
// reconstruct part of the fused frame kernel (fs_frame.hip).  kWarm: fs_internal.hpp.
// A publish without the host's help: the reconstruct workgroups of a launch write the channel views straight into the sources'
// pinned host ring slots; every one of them, once its stores have been acknowledged, takes a ticket, and the workgroup that takes
// the last one stores the launch's id into the context's pinned host word — fs_get_impulse_response* and the ring's back-pressure
// read that word: no event, no copy command, no second stream (fs_capi_publish.cpp: owed_publish).  The ticket cell re-arms itself.
// The samples go to the host with SYSTEM-scope stores (store_sys: sc0 sc1 — written through to the host before they are
// acknowledged), so a wave whose store counter has run out (s_waitcnt vmcnt(0): on gfx9 stores count there too) knows that its
// samples are where the host reads them; the barrier collects the workgroup's waves, the tickets the launch's workgroups, and the
// word — a system-scope store as well — is issued only then: it can never overtake the samples.  Two things that do NOT work:
// plain stores + the counter (the word overtook the samples: tests/test_round3.py's stream of grouped frames read 6 of 7
// publishes too early — plain stores to fine-grained memory are acknowledged by the L2, not by the host), and a system-scope
// FENCE per wave (__threadfence_system(): correct, but it also writes back every dirty L2 line of the chip each time: the 3 072
// reconstruct workgroups of a 128-source tick paid 0.27 ms for it, the fused frame kernel 3 %).
__device__ __forceinline__ void store_sys(float* p, const float4 v) {   // 16 bytes, system scope (p 16-byte aligned)
    typedef float sys_v4f __attribute__((ext_vector_type(4)));
    const sys_v4f x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(x) : "memory");
}
__device__ __forceinline__ void store_sys(float* p, const float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void publish_arrive(unsigned* __restrict__ tickets, unsigned total, unsigned long long* __restrict__ host_word,
                                               unsigned long long id) {
    if (tickets == nullptr) return;                       // (uniform: this launch is published through an event)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(tickets, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t + 1u == total) {
            __hip_atomic_store(tickets, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the next launch of the stream starts behind this one)
            __hip_atomic_store(host_word, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// host_out (optional, row B only): the block's samples also go to that pinned host buffer, staged in `s_stage`
// (kBlock x (kChunk + 1) floats of LDS) and written with one 16-byte store per lane and instruction.
// ir_bands == nullptr (a frame whose IR is superseded within its own launch): only the channel row is produced, for the host.
// The zero-block rule of the host slot (slot_mask: one device word per ring slot, bit b = block b of the slot may hold non-zero
// samples).  A block none of whose reachable amplitudes (its bins, the bin before, the kWarm run-in) is non-zero produces exact
// zeros: it is written across the bus only if the slot still holds something else there.  A room's IR ends after 60 - 230 of the
// 1000 bins: 9 - 10 of a slot's 12 blocks stay on the device side of the bus (the 128-source tick wrote 24.6 MB per tick).
// Returns whether this workgroup must write its block to the host; every thread of the workgroup must call it.
// (the two halves of the rule: this thread's share of the reach test, then the workgroup's vote and the mask bit)
__device__ __forceinline__ bool block_reach_nonzero(const float* s_amp, int nb, int spb, int base) {
    const int b0 = max((base - kWarm) / spb - 1, 0), b1 = min((base + kReconBlockSamples - 1) / spb, nb - 1);
    bool nz = false;
    for (int b = b0 + (int)threadIdx.x; b <= b1; b += kBlock) nz = nz || s_amp[b] != 0.0f;
    return nz;
}
__device__ __forceinline__ bool host_block_vote(bool nz, int block, uint32_t* __restrict__ slot_mask) {
    const bool any = __syncthreads_or(nz ? 1 : 0) != 0;
    const uint32_t bit = 1u << block;
    const bool dirty = (__hip_atomic_load(slot_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) != 0u;   // (only this workgroup touches this bit)
    __syncthreads();                                        // (everybody has read the word before thread 0 rewrites it)
    if (threadIdx.x == 0) {
        if (any && !dirty) __hip_atomic_fetch_or(slot_mask, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!any && dirty) __hip_atomic_fetch_and(slot_mask, ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return any || dirty;
}
__device__ __forceinline__ bool host_block_wanted(const float* s_amp, int nb, int spb, int base, int block, uint32_t* __restrict__ slot_mask) {
    if (slot_mask == nullptr) return true;
    return host_block_vote(block_reach_nonzero(s_amp, nb, spb, base), block, slot_mask);
}

__device__ __forceinline__ void reconstruct_body(const int row, const int chunk_block, const float* __restrict__ energy, int B, int nb,
                                                 int num_samples, int spb, float* __restrict__ ir_bands,
                                                 float* __restrict__ ir_mono, float* s_amp, float* host_out = nullptr,
                                                 float* s_stage = nullptr, uint32_t* __restrict__ slot_mask = nullptr) {
    const float Pi4 = sqrtf(4.0f * kPi);                           // FSAC.cpp:323
    if (ir_bands == nullptr && (row < B || host_out == nullptr)) return;   // (uniform) nobody wants this row
    for (int i = threadIdx.x; i < nb; i += kBlock) {
        float e;
        if (row < B) e = energy[row * nb + i];
        else {
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += energy[b * nb + i];
            e = s / (float)B;
        }
        float a = 0.0f;
        if (fabsf(e) >= 1e-6f) a = e / sqrtf(e * Pi4);             // FSAC.cpp:343-345
        s_amp[i] = a;
    }
    __syncthreads();
    const int chunk = chunk_block * kBlock + threadIdx.x;
    const int s0 = chunk * kChunk;
    bool to_host = host_out != nullptr && row == B;         // (uniform for the workgroup)
    if (to_host) to_host = host_block_wanted(s_amp, nb, spb, chunk_block * kBlock * kChunk, chunk_block, slot_mask);
    const bool staged = s_stage != nullptr;                 // (uniform) the block's samples leave through LDS: 16-byte stores of consecutive lanes
    if (s0 >= num_samples && !staged) return;
    float* out = ir_bands == nullptr ? nullptr : (row < B ? ir_bands + (size_t)row * num_samples : ir_mono);   // (nullptr: staged, host only)
    const int s1 = min(s0 + kChunk, num_samples);        // (a thread beyond the end: an empty range, it only joins the barrier below)
    const int i0 = s0 < num_samples ? max(s0 - kWarm, 0) : s1;
    int bin = i0 / spb;
    int bs = i0 - bin * spb;
    float cur = bin < nb ? s_amp[bin] : 0.0f;
    float prev = bin == 0 ? cur : (bin - 1 < nb ? s_amp[bin - 1] : 0.0f);   // FSAC.cpp:347-355
    const float fspb = (float)spb;
    float y = 0.0f;
    for (int i = i0; i < s1; ++i) {
        float x = 0.0f;
        if (bin < nb) {
            float wgt = (float)bs / fspb;                           // FSAC.cpp:359
            float a = (1.0f - wgt) * prev;
            float b = wgt * cur;
            x = a + b;                                              // FSAC.cpp:360
        }
        if (i == 0) {
            y = x;                                                  // Filtered[0] = IR[0] FSAC.cpp:371
        } else {
            float a = 0.25f * x;
            float b = (1.0f - 0.25f) * y;
            y = a + b;                                              // FSAC.cpp:374
        }
        if (i >= s0) {
            // (a thread's own 16 samples lie 64 bytes from its neighbour's: stored one by one, every store instruction of a wave
            // touches 64 lines — 20 of the 26 us of a one-source reconstruct, the same again for the host copy)
            if (staged) s_stage[threadIdx.x * (kChunk + 1) + (i - s0)] = y;   // (+ 1: conflict-free rows)
            else if (out) out[i] = y;
        }
        if (++bs == spb) {
            bs = 0;
            ++bin;
            prev = cur;
            cur = bin < nb ? s_amp[bin] : 0.0f;
        }
    }
    if (staged) {   // the block's kBlock * kChunk consecutive samples, 16 bytes per lane: to the device array, and the channel row to the host slot
        __syncthreads();
        const int base = chunk_block * kBlock * kChunk;
        for (int v = threadIdx.x; v < kBlock * kChunk / 4; v += kBlock) {
            const int s = 4 * v;
            if (base + s + 3 < num_samples) {
                float4 o;   // (sample s of the block lives in row s / kChunk of kChunk + 1 words)
                o.x = s_stage[s + s / kChunk]; o.y = s_stage[s + 1 + (s + 1) / kChunk];
                o.z = s_stage[s + 2 + (s + 2) / kChunk]; o.w = s_stage[s + 3 + (s + 3) / kChunk];
                if (out) *reinterpret_cast<float4*>(out + base + s) = o;
                if (to_host) store_sys(host_out + base + s, o);
            } else {
                for (int e = 0; e < 4; ++e)
                    if (base + s + e < num_samples) {
                        const float y1 = s_stage[s + e + (s + e) / kChunk];
                        if (out) out[base + s + e] = y1;
                        if (to_host) store_sys(host_out + base + s + e, y1);
                    }
            }
        }
    }
}

// The same reconstruct for the kernels that only reconstruct (reconstruct_kernel, reconstruct_batch_kernel), in two phases.  In
// reconstruct_body a thread's 16 samples cost it a chain of 16 + kWarm interpolated samples — a division, four branches and
// their bookkeeping each, ~ 60 instructions a sample on a wave that is alone on its SIMD: 20 of the 26 us of a one-source
// reconstruct (the stores, scattered or not, to the device or to the host, were 2 of them: profiles/r04 notes in DESIGN.md).
// Here every interpolated sample of the block (and of the kWarm before it) is computed ONCE, by the thread that owns it, into
// LDS; the filter chain then reads them: three arithmetic instructions a sample.  The same operations on the same operands in
// the same order as reconstruct_body: the same bits.
// LDS: s_amp [nb] | s_x [kBlock * kChunk + kWarm] | s_stage [kBlock][kChunk + 1].

// The phases of reconstruct_body_fast, shared with the spectral channel row (reconstruct_spectral_row) so that its band envelopes
// are the band rows' own bits.  The amplitudes of one row: row < B a band, row == B the band mean.
__device__ __forceinline__ void recon_amplitudes(const int row, const float* __restrict__ energy, int B, int nb, float* s_amp) {
    const float Pi4 = sqrtf(4.0f * kPi);                           // FSAC.cpp:323
    for (int i = threadIdx.x; i < nb; i += kBlock) {
        float e;
        if (row < B) e = energy[row * nb + i];
        else {
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += energy[b * nb + i];
            e = s / (float)B;
        }
        float a = 0.0f;
        if (fabsf(e) >= 1e-6f) a = e / sqrtf(e * Pi4);             // FSAC.cpp:343-345
        s_amp[i] = a;
    }
}
// Where sample i of s_x lives.  PAD: one spare word behind every kChunk samples.  A thread's chain starts at a multiple of kChunk,
// so without the pad the lanes of a wave are kChunk = 16 words apart in every read of the filter and every write of the
// interpolation: two of the 32 banks of a ds_read_b32 / ds_write_b32, 16 lanes on each.  A kernel that only reconstructs does not
// notice (nobody else wants its CU's LDS); a reconstruct workgroup of the fused frame kernel shares its CU with walk waves whose
// stack pushes and pops are on their critical chain.  17 words apart, the 32 lanes of a half wave hit 32 banks.
template <bool PAD> __device__ __forceinline__ constexpr int recon_x_pos(int i) { return PAD ? i + i / kChunk : i; }
static_assert(kWarm % kChunk == 0, "a filter chain starts at a multiple of kChunk samples of s_x");
// phase 1: the interpolated samples x[base - kWarm .. base + kBlock * kChunk) -> s_x[0 ..): thread t its own kChunk, and the
// first kWarm threads one sample each of the run-in (samples before 0 do not exist: never read)
template <bool PAD = false>
__device__ __forceinline__ void recon_interpolate(const int base, int nb, int spb, const float* s_amp, float* s_x) {
    const float fspb = (float)spb;
    auto interp = [&](int i) {
        const int bin = i / spb, bs = i - bin * spb;
        float x = 0.0f;
        if (bin < nb) {
            const float cur = s_amp[bin];
            const float prev = bin == 0 ? cur : s_amp[bin - 1];         // FSAC.cpp:347-355
            const float wgt = (float)bs / fspb;                          // FSAC.cpp:359
            const float a = (1.0f - wgt) * prev;
            const float b = wgt * cur;
            x = a + b;                                                   // FSAC.cpp:360
        }
        return x;
    };
    const int s0 = base + (int)threadIdx.x * kChunk;
    int bin = s0 / spb, bs = s0 - bin * spb;                     // (incrementally within the thread's own samples: no division by spb per sample)
    float cur = bin < nb ? s_amp[bin] : 0.0f;
    float prev = bin == 0 ? cur : (bin - 1 < nb ? s_amp[bin - 1] : 0.0f);
#pragma unroll 4
    for (int e = 0; e < kChunk; ++e) {
        float x = 0.0f;
        if (bin < nb) {
            const float wgt = (float)bs / fspb;
            const float a = (1.0f - wgt) * prev;
            const float b = wgt * cur;
            x = a + b;
        }
        s_x[recon_x_pos<PAD>(kWarm + (int)threadIdx.x * kChunk) + e] = x;
        if (++bs == spb) { bs = 0; ++bin; prev = cur; cur = bin < nb ? s_amp[bin] : 0.0f; }
    }
    if ((int)threadIdx.x < kWarm) {
        const int i = base - kWarm + (int)threadIdx.x;
        s_x[recon_x_pos<PAD>((int)threadIdx.x)] = i >= 0 ? interp(i) : 0.0f;
    }
}
// phase 2: the one-pole filter over this thread's kChunk samples behind a run-in of kWarm (0.75^96 ~ 1e-12); `my` = the thread's
// kChunk outputs: a row of LDS, or — every index a constant — an array that stays in registers.  The chain is read in groups of
// kChunk samples (whole groups: s0 and kWarm are multiples of kChunk), each at constant offsets from the group's position.
template <bool PAD = false>
__device__ __forceinline__ void recon_filter(const int base, const float* s_x, float* my) {
    const int s0 = base + (int)threadIdx.x * kChunk;
    const int i0 = max(s0 - kWarm, 0);                           // global index of the first sample of the chain
    const int at = i0 - (base - kWarm);                          // x[i0] is sample `at` of s_x
    const int run = s0 - i0;                                     // kWarm, less at the very beginning of the IR
    float y = 0.0f;
    bool first = i0 == 0;                                        // Filtered[0] = IR[0] FSAC.cpp:371 (the first threads of the first block)
    for (int g = 0; g < run; g += kChunk) {
        const float* xs = s_x + recon_x_pos<PAD>(at + g);
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            const float a = 0.25f * xs[k]; const float b = (1.0f - 0.25f) * y; const float f = a + b;   // FSAC.cpp:374
            y = (k == 0 && first) ? xs[0] : f;
        }
        first = false;
    }
    const float* own = s_x + recon_x_pos<PAD>(at + run);         // the thread's own samples
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
        const float a = 0.25f * own[k]; const float b = (1.0f - 0.25f) * y; const float f = a + b;
        y = (k == 0 && first) ? own[0] : f;                      // (sample 0 of the IR is its own output)
        my[k] = y;
    }
}
// the block's kBlock * kChunk consecutive samples from s_stage, 16 bytes per lane: the device array, and the channel row to the host slot
__device__ __forceinline__ void recon_store(const int base, int num_samples, const float* s_stage, float* __restrict__ out, bool to_host,
                                            float* host_out) {
    for (int v = threadIdx.x; v < kBlock * kChunk / 4; v += kBlock) {
        const int sidx = 4 * v;
        if (base + sidx + 3 < num_samples) {
            float4 o;
            o.x = s_stage[sidx + sidx / kChunk]; o.y = s_stage[sidx + 1 + (sidx + 1) / kChunk];
            o.z = s_stage[sidx + 2 + (sidx + 2) / kChunk]; o.w = s_stage[sidx + 3 + (sidx + 3) / kChunk];
            if (out) *reinterpret_cast<float4*>(out + base + sidx) = o;
            if (to_host) store_sys(host_out + base + sidx, o);
        } else {
            for (int e = 0; e < 4; ++e)
                if (base + sidx + e < num_samples) {
                    const float y1 = s_stage[sidx + e + (sidx + e) / kChunk];
                    if (out) out[base + sidx + e] = y1;
                    if (to_host) store_sys(host_out + base + sidx + e, y1);
                }
        }
    }
}

__device__ __forceinline__ void reconstruct_body_fast(const int row, const int chunk_block, const float* __restrict__ energy, int B, int nb,
                                                      int num_samples, int spb, float* __restrict__ ir_bands, float* __restrict__ ir_mono,
                                                      float* s_amp, float* host_out, uint32_t* __restrict__ slot_mask = nullptr) {
    float* s_x = s_amp + nb;
    float* s_stage = s_x + kBlock * kChunk + kWarm;
    if (ir_bands == nullptr && (row < B || host_out == nullptr)) return;   // (uniform) a superseded frame: only its channel row, for the host
    recon_amplitudes(row, energy, B, nb, s_amp);
    __syncthreads();
    bool to_host = host_out != nullptr && row == B;         // (uniform for the workgroup)
    float* out = ir_bands == nullptr ? nullptr : (row < B ? ir_bands + (size_t)row * num_samples : ir_mono);
    const int base = chunk_block * kBlock * kChunk;          // the block's first sample
    if (to_host) to_host = host_block_wanted(s_amp, nb, spb, base, chunk_block, slot_mask);
    recon_interpolate(base, nb, spb, s_amp, s_x);
    __syncthreads();
    recon_filter(base, s_x, s_stage + threadIdx.x * (kChunk + 1));   // (+ 1: conflict-free rows)
    __syncthreads();
    recon_store(base, num_samples, s_stage, out, to_host, host_out);
}

// The two phases for the reconstruct part of the narrow fused frame kernels (fs_frame.hip), in hardly more LDS than the one-phase
// body took there (reconstruct_body_fast's 38 KB would have been the launch's largest part): the filter's kChunk outputs wait in
// registers until every chain of the workgroup has read its samples, and the staging rows then take the place of the
// interpolated samples.  The same phases as reconstruct_body_fast: the same bits.
// LDS: s_amp [nb] | s_x [kBlock * kChunk + kWarm] with a pad word per kChunk (recon_x_pos), later s_stage [kBlock][kChunk + 1]:
// fs_internal.hpp: frame_recon_lds_bytes.
__device__ __forceinline__ void reconstruct_body_staged(const int row, const int chunk_block, const float* __restrict__ energy, int B, int nb,
                                                        int num_samples, int spb, float* __restrict__ ir_bands, float* __restrict__ ir_mono,
                                                        float* s_amp, float* host_out, uint32_t* __restrict__ slot_mask = nullptr) {
    float* s_x = s_amp + nb;
    if (ir_bands == nullptr && (row < B || host_out == nullptr)) return;   // (uniform) a superseded frame: only its channel row, for the host
    recon_amplitudes(row, energy, B, nb, s_amp);
    __syncthreads();
    bool to_host = host_out != nullptr && row == B;         // (uniform for the workgroup)
    float* out = ir_bands == nullptr ? nullptr : (row < B ? ir_bands + (size_t)row * num_samples : ir_mono);
    const int base = chunk_block * kBlock * kChunk;          // the block's first sample
    if (to_host) to_host = host_block_wanted(s_amp, nb, spb, base, chunk_block, slot_mask);
    recon_interpolate<true>(base, nb, spb, s_amp, s_x);
    __syncthreads();
    float y[kChunk];
    recon_filter<true>(base, s_x, y);
    __syncthreads();                                         // (every chain has read its samples: the area becomes the staging rows)
    float* my = s_x + threadIdx.x * (kChunk + 1);            // (+ 1: conflict-free rows)
#pragma unroll
    for (int e = 0; e < kChunk; ++e) my[e] = y[e];
    __syncthreads();
    recon_store(base, num_samples, s_x, out, to_host, host_out);
}

// FS_FLAG_SPECTRAL_IR: the channel row (row B) as y[n] = (1/sqrt(B)) sum_b env_b[n] c_b[n] — env_b = band row b, bit for bit (the
// phases above), c_b = the band's unit-power noise carrier ([B][carrier_stride(num_samples)] fp32, fs_fft.hip: launch_build_carriers).
// The workgroup computes every band's envelope for its own block (no other workgroup's band row is read: the rows' workgroups are
// not ordered, and a superseded frame has no band rows at all).  The products are summed over the bands in registers, the carrier
// read as 16-byte loads of the thread's kChunk samples.  Zero blocks: a block is non-zero if ANY band's amplitude in its reach is
// (one band above the 1e-6 cut can leave the band MEAN below it); where every envelope is zero the output is an exact zero.
// Used by the fused frame kernel and by the reconstruct-only kernels alike: the same bits on every route.
// LDS: reconstruct_body_staged's layout (a band's envelope goes from the filter to the products in registers; the staging rows
// are written once, behind the last band's barrier, where the interpolated samples were).
__device__ __forceinline__ void reconstruct_spectral_row(const int chunk_block, const float* __restrict__ energy, int B, int nb,
                                                         int num_samples, int spb, float* __restrict__ ir_bands, float* __restrict__ ir_mono,
                                                         float* s_amp, float* host_out, uint32_t* __restrict__ slot_mask,
                                                         const float* __restrict__ carrier) {
    float* s_x = s_amp + nb;
    float* s_stage = s_x;
    if (ir_bands == nullptr && host_out == nullptr) return;   // (uniform) nobody wants this row
    float* out = ir_bands == nullptr ? nullptr : ir_mono;
    const int base = chunk_block * kBlock * kChunk;
    const int s0 = base + (int)threadIdx.x * kChunk;
    const size_t ld = (size_t)carrier_stride(num_samples);
    float* my = s_stage + threadIdx.x * (kChunk + 1);
    float acc[kChunk], env[kChunk];
#pragma unroll
    for (int e = 0; e < kChunk; ++e) acc[e] = 0.0f;
    bool nz = false;
    for (int band = 0; band < B; ++band) {
        recon_amplitudes(band, energy, B, nb, s_amp);
        __syncthreads();
        nz = nz || block_reach_nonzero(s_amp, nb, spb, base);
        recon_interpolate<true>(base, nb, spb, s_amp, s_x);
        __syncthreads();
        recon_filter<true>(base, s_x, env);                          // env_b of the thread's kChunk samples
        if (s0 < num_samples) {
            const float4* c = reinterpret_cast<const float4*>(carrier + (size_t)band * ld + s0);   // (ld and s0: multiples of kChunk: 16-byte aligned)
#pragma unroll
            for (int q = 0; q < kChunk / 4; ++q) {
                const float4 cv = c[q];
                acc[4 * q + 0] = acc[4 * q + 0] + env[4 * q + 0] * cv.x;
                acc[4 * q + 1] = acc[4 * q + 1] + env[4 * q + 1] * cv.y;
                acc[4 * q + 2] = acc[4 * q + 2] + env[4 * q + 2] * cv.z;
                acc[4 * q + 3] = acc[4 * q + 3] + env[4 * q + 3] * cv.w;
            }
        }
        __syncthreads();                                        // (the next band rewrites s_amp and s_x)
    }
    const float g = 1.0f / sqrtf((float)B);
#pragma unroll
    for (int e = 0; e < kChunk; ++e) my[e] = acc[e] * g;
    bool to_host = host_out != nullptr;
    if (to_host && slot_mask != nullptr) to_host = host_block_vote(nz, chunk_block, slot_mask);   // (its barriers order the rows above)
    __syncthreads();
    recon_store(base, num_samples, s_stage, out, to_host, host_out);
}

// FS_FLAG_ROOM_PARAMETERS: the room parameters of one band of a histogram, one workgroup (definitions: DESIGN.md section 8, "Room
// parameters"; include/frequensee.h fs_room_parameters).  Everything in double, rounded to float once.  The row is read once into
// LDS; thread t owns the contiguous bins [t per, (t + 1) per).  Every sum is a chunk sum in bin order followed by a fixed-order
// tree over the threads (room_reduce), so the same row gives the same bits on every run and every route.  The Schroeder sum
// S[k] = R_t + (the chunk's own suffix), R_t = the exclusive suffix scan of the chunk sums; each pass that needs L[k] walks its
// chunk backwards and recomputes S[k] with the same operations (no [num_bins] doubles in LDS).
// LDS: s_e [num_bins] floats | s_d [kRoomRows][kBlock] doubles + one broadcast slot (room_lds_bytes).  Thread 0 writes the record
// `out` (kRoomFields floats of pinned host memory) with system-scope stores: the launch may publish right behind it.
template <int NV, typename Op>
__device__ __forceinline__ void room_reduce(double* s_d, Op op) {   // rows 0 .. NV-1 of s_d: after the call s_d[v * kBlock] = row v reduced
    for (int stride = kBlock / 2; stride > 0; stride >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < stride)
#pragma unroll
            for (int v = 0; v < NV; ++v) s_d[v * kBlock + threadIdx.x] = op(s_d[v * kBlock + threadIdx.x], s_d[v * kBlock + threadIdx.x + stride]);
    }
    __syncthreads();
}
__device__ __forceinline__ void room_parameters_band(const float* __restrict__ row, int nb, float bin_duration, float* out, float* s_lds) {
    float* s_e = s_lds;
    double* s_d = reinterpret_cast<double*>(s_lds + ((nb + 1) & ~1));
    double* s_bc = s_d + kRoomRows * kBlock;                  // broadcast slot: S[k0]
    const int t = (int)threadIdx.x;
    for (int k = t; k < nb; k += kBlock) s_e[k] = row[k];
    __syncthreads();
    const int per = (nb + kBlock - 1) / kBlock;
    const int k_lo = min(t * per, nb), k_hi = min(k_lo + per, nb);
    // the energy, the peak, the validity
    double csum = 0.0;
    float cmax = 0.0f;
    bool bad = false, pos = false;
    for (int k = k_lo; k < k_hi; ++k) {
        const float e = s_e[k];
        bad = bad || !(e >= 0.0f) || e == INFINITY;              // negative, NaN or infinite
        pos = pos || e > 0.0f;
        cmax = fmaxf(cmax, e);
        csum += (double)e;
    }
    s_d[t] = csum;
    s_d[kBlock + t] = (double)cmax;
    room_reduce<1>(s_d, [](double a, double b) { return a + b; });
    const double energy = s_d[0];
    __syncthreads();
    room_reduce<1>(s_d + kBlock, [](double a, double b) { return a > b ? a : b; });
    const double pk = s_d[kBlock];
    const bool invalid = __syncthreads_or(bad ? 1 : 0) != 0 || __syncthreads_or(pos ? 1 : 0) == 0;
    if (invalid) {   // (uniform)
        if (t == 0) {
            store_sys(out, (float)energy);
            for (int f = 1; f < kRoomFields; ++f) store_sys(out + f, __int_as_float(0x7FC00000));
        }
        return;
    }
    // the onset: the first bin within 20 dB of the peak (a min-index reduction)
    const double thr = pk / 100.0;
    int first = nb;
    for (int k = k_lo; k < k_hi && first == nb; ++k) if ((double)s_e[k] >= thr) first = k;
    s_d[t] = (double)first;
    room_reduce<1>(s_d, [](double a, double b) { return a < b ? a : b; });
    const int k0 = (int)s_d[0];
    __syncthreads();
    // R_t: the exclusive suffix scan of the chunk sums (Hillis-Steele over two rows of s_d)
    s_d[t] = csum;
    double* src = s_d;
    double* dst = s_d + kBlock;
    for (int d = 1; d < kBlock; d <<= 1) {
        __syncthreads();
        dst[t] = t + d < kBlock ? src[t] + src[t + d] : src[t];
        double* x = src; src = dst; dst = x;
    }
    __syncthreads();
    const double R = t + 1 < kBlock ? src[t + 1] : 0.0;
    __syncthreads();
    // S[k0] (by the thread that owns k0)
    if (k0 >= k_lo && k0 < k_hi) {
        double inner = 0.0;
        for (int k = k_hi - 1; k >= k0; --k) inner += (double)s_e[k];
        *s_bc = R + inner;
    }
    __syncthreads();
    const double S0 = *s_bc;
    const double dt = (double)bin_duration;
    const double lo[3] = {-10.0, -25.0, -35.0}, hi[3] = {0.0, -5.0, -5.0};   // edt, t20, t30
    // pass A: fit points (count, sum t, sum L), "the decay leaves the range", early / late energy, sum t E
    double n[3] = {0.0, 0.0, 0.0}, st[3] = {0.0, 0.0, 0.0}, sl[3] = {0.0, 0.0, 0.0};
    bool below[3] = {false, false, false};
    double e50 = 0.0, l50 = 0.0, e80 = 0.0, l80 = 0.0, te = 0.0;
    {
        double inner = 0.0;
        for (int k = k_hi - 1; k >= k_lo && k >= k0; --k) {
            const double e = (double)s_e[k];
            inner += e;
            const double S = R + inner;
            const double L = S > 0.0 ? 10.0 * log10(S / S0) : -INFINITY;
            const double tk = (double)(k - k0) * dt;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                if (L >= lo[r] && L <= hi[r]) { n[r] += 1.0; st[r] += tk; sl[r] += L; }
                below[r] = below[r] || L < lo[r];
            }
            if (tk < 0.050) e50 += e; else l50 += e;
            if (tk < 0.080) e80 += e; else l80 += e;
            te += tk * e;
        }
    }
    {
        const double v[kRoomRows] = {n[0], n[1], n[2], st[0], st[1], st[2], sl[0], sl[1], sl[2], e50, l50, e80, l80, te};
#pragma unroll
        for (int i = 0; i < kRoomRows; ++i) s_d[i * kBlock + t] = v[i];
    }
    room_reduce<kRoomRows>(s_d, [](double a, double b) { return a + b; });
    double sum[kRoomRows];
#pragma unroll
    for (int i = 0; i < kRoomRows; ++i) sum[i] = s_d[i * kBlock];
    bool leaves[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) leaves[r] = __syncthreads_or(below[r] ? 1 : 0) != 0;   // (also the barrier before s_d is rewritten)
    double tbar[3], lbar[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { tbar[r] = sum[3 + r] / sum[r]; lbar[r] = sum[6 + r] / sum[r]; }
    // pass B: the centred sums of the three fits
    double sxy[3] = {0.0, 0.0, 0.0}, sxx[3] = {0.0, 0.0, 0.0};
    {
        double inner = 0.0;
        for (int k = k_hi - 1; k >= k_lo && k >= k0; --k) {
            inner += (double)s_e[k];
            const double S = R + inner;
            const double L = S > 0.0 ? 10.0 * log10(S / S0) : -INFINITY;
            const double tk = (double)(k - k0) * dt;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (L >= lo[r] && L <= hi[r]) {
                    const double a = tk - tbar[r], b = L - lbar[r];
                    sxy[r] += a * b;
                    sxx[r] += a * a;
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) { s_d[r * kBlock + t] = sxy[r]; s_d[(3 + r) * kBlock + t] = sxx[r]; }
    room_reduce<6>(s_d, [](double a, double b) { return a + b; });
    if (t == 0) {
        const float qnan = __int_as_float(0x7FC00000);
        float T[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double m = s_d[r * kBlock] / s_d[(3 + r) * kBlock];
            T[r] = (sum[r] < 2.0 || !leaves[r] || !(m < 0.0)) ? qnan : (float)(-60.0 / m);
        }
        const double e50s = sum[9], l50s = sum[10], e80s = sum[11], l80s = sum[12];
        store_sys(out + 0, (float)energy);
        store_sys(out + 1, (float)((double)k0 * dt));
        store_sys(out + 2, T[0]);
        store_sys(out + 3, T[1]);
        store_sys(out + 4, T[2]);
        store_sys(out + 5, l50s > 0.0 ? (float)(10.0 * log10(e50s / l50s)) : INFINITY);
        store_sys(out + 6, l80s > 0.0 ? (float)(10.0 * log10(e80s / l80s)) : INFINITY);
        store_sys(out + 7, (float)(e50s / (e50s + l50s)));
        store_sys(out + 8, (float)(sum[13] / (e50s + l50s)));
    }
}

}  // namespace
}  // namespace fs
