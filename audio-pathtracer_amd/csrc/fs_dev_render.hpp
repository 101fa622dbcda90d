// fs_dev_render.hpp — what the four render kernels of the audio thread (fs_direct_render.hip, fs_reflect_render.hip,
// fs_binaural_render.hip, fs_ambisonic_render.hip) share on the device: one voice's block — a time-varying fractional delay and a linear-phase FIR whose
// taps ramp from sum_b g0_b k_b to sum_b g1_b k_b — as pieces a kernel puts together: the delay of an output sample and its slew
// clamp, the tap table and the tile's read window in LDS, the tap loop of one output sample, the output store with the ring append.
// Behind them the voice bank, which the reflection, the binaural and the ambisonic renderer are: the plan pass and the render pass
// of a callback whose rows hold a table of voices, with what a renderer's voices carry beyond a delay and band gains, and where
// their taps come from, handed in (the ambisonic renderer has a render pass of its own: one voice evaluation for all channels).
// The rule is
// include/frequensee.h's, to the bit: every fp32 operation stands where the header puts it (the files are built with
// -ffp-contract=off and the tests compare bits).  No piece of a voice's block holds a barrier or a return: each says which barrier
// its caller owes.  The LDS arrays travel as references to arrays, so that after inlining the tap loop still reads them with LDS
// instructions.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fs_internal.hpp"

namespace fs {
namespace {

constexpr int kRenderTile = 256;                               // outputs per workgroup = threads per workgroup
constexpr int kRenderMaxTaps = FS_DIRECT_RENDER_MAX_TAPS;
// the window of a tile: its outputs, the taps, x(p - 1), and the delay's travel across the tile — the slew limit bounds that
// to half a sample per sample, plus one for the floor
constexpr int kRenderWindow = kRenderTile + kRenderTile / 2 + kRenderMaxTaps + 8;
using RenderTaps = float2[kRenderMaxTaps + 1];   // {c0[t], dc[t]}
using RenderWindow = float[kRenderWindow];

// the delay of output sample s: a = (s + 1) / F, d = d0 + a e
__device__ __forceinline__ float render_delay(float d0, float e, int s, float frame_f, float* a_out) {
    const float a = (float)(s + 1) / frame_f;
    *a_out = a;
    return d0 + a * e;
}

// the slew limit of a callback's change of delay: half a sample per sample
__device__ __forceinline__ float render_slew(float e, int frame) {
    const float half = 0.5f * (float)frame;
    if (e < -half) e = -half;
    if (e > half) e = half;
    return e;
}

// {c0[t], c1[t] - c0[t]}, c = sum_b g_b k_b, into s_cd.  The caller owes a barrier between this and the first render_sample, and
// one between the last render_sample and the next build.
__device__ __forceinline__ void render_build_taps(RenderTaps& s_cd, const float* __restrict__ table, const float* __restrict__ g0,
                                                  const float* __restrict__ g1, int taps, int bands, int tid) {
    for (int t = tid; t < taps; t += kRenderTile) {
        float c0 = 0.0f, c1 = 0.0f;
        for (int b = 0; b < bands; ++b) {
            const float k = table[(size_t)b * (size_t)taps + t];
            c0 = c0 + g0[b] * k;
            c1 = c1 + g1[b] * k;
        }
        s_cd[t] = make_float2(c0, c1 - c0);
    }
}

// What a ring holds of a row's interleaved stereo block `in`, as sample rel of the block: one of its channels (the direct, the
// reflection and the binaural renderer: a ring per channel), or the downmix of a mono source (the ambisonic renderer: one ring)
struct RenderChannel {
    const float* __restrict__ in;
    int ch;
    __device__ __forceinline__ float operator()(int rel) const { return in[2 * rel + ch]; }
};
struct RenderDownmix {
    const float* __restrict__ in;
    __device__ __forceinline__ float operator()(int rel) const { return 0.5f * (in[2 * rel] + in[2 * rel + 1]); }
};

// The read window of the tile's outputs [s_a, s_b] into s_win, from the ring (samples before n0) and the block (from n0 on, read
// through x_in; past the block's end: 0).  Returns i_hi, the largest whole delay of the tile, which places a sample's taps
// in the window (render_sample).  The same barriers as render_build_taps.
template <typename In>
__device__ __forceinline__ int render_stage_window(RenderWindow& s_win, const float* __restrict__ ring, unsigned mask, const In& x_in,
                                                   unsigned n0, float d0, float e, int s_a, int s_b, int frame, float frame_f, int taps,
                                                   int tid) {
    // d is monotone in s (every rounding is), so the tile's whole delays lie between those of its first and last output
    float a_unused;
    const int i_a = (int)floorf(render_delay(d0, e, s_a, frame_f, &a_unused));
    const int i_b = (int)floorf(render_delay(d0, e, s_b, frame_f, &a_unused));
    const int i_lo = min(i_a, i_b), i_hi = max(i_a, i_b);
    const unsigned p_lo = n0 + (unsigned)s_a - (unsigned)(taps - 1) - (unsigned)i_hi - 1u;   // absolute index of s_win[0]
    const int wlen = min((s_b - s_a) + (i_hi - i_lo) + taps + 1, kRenderWindow);
    for (int j = tid; j < wlen; j += kRenderTile) {
        const unsigned p = p_lo + (unsigned)j;
        const int rel = (int)(p - n0);   // >= 0: a sample of this block
        float v = 0.0f;
        if (rel < 0) v = ring[p & mask];
        else if (rel < frame) v = x_in(rel);
        s_win[j] = v;
    }
    return i_hi;
}
// ... of channel ch of the block
__device__ __forceinline__ int render_stage_window(RenderWindow& s_win, const float* __restrict__ ring, unsigned mask,
                                                   const float* __restrict__ in, int ch, unsigned n0, float d0, float e, int s_a, int s_b, int frame,
                                                   float frame_f, int taps, int tid) {
    return render_stage_window(s_win, ring, mask, RenderChannel{in, ch}, n0, d0, e, s_a, s_b, frame, frame_f, taps, tid);
}

// Output sample s < frame of the voice whose taps and window the LDS holds: the four-accumulator tap loop, (acc0 + acc1) +
// (acc2 + acc3); *a_out = the sample's ramp position.  c0 / dc are wave-uniform broadcasts, neighbouring lanes read neighbouring
// samples, x(p - 1) of tap t is x(p) of tap t + 1 (one sample read per tap).  Behind the barrier that follows the build and the
// staging.
__device__ __forceinline__ float render_sample(const RenderTaps& s_cd, const RenderWindow& s_win, float d0, float e, int s, int s_a,
                                               int i_hi, float frame_f, int taps, float* a_out) {
    float a;
    const float d = render_delay(d0, e, s, frame_f, &a);
    *a_out = a;
    const float fl = floorf(d);
    const int i = (int)fl;
    const float f = d - fl;
    // tap t reads x(p) = s_win[base - t] and x(p - 1) = s_win[base - t - 1], p = n0 + s - t - i
    const int base = min((s - s_a) + (i_hi - i) + taps, kRenderWindow - 1);
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
    return (acc0 + acc1) + (acc2 + acc3);
}

// Sample s < frame of the block, read through x_in, into the ring.  A callback reads ring positions [n0 - D - T, n0) and writes
// [n0, n0 + F), disjoint modulo the ring because it holds D + T + 1 + F or more: no barrier.
template <typename In>
__device__ __forceinline__ void render_append(float* __restrict__ ring, unsigned mask, const In& x_in, unsigned n0, int s) {
    ring[(n0 + (unsigned)s) & mask] = x_in(s);
}

// Output sample s < frame of row r: y into out, the input sample of channel ch into the ring.
__device__ __forceinline__ void render_store(float* __restrict__ out_all, float* __restrict__ ring, unsigned mask,
                                             const float* __restrict__ in, int r, int ch, unsigned n0, int s, int frame, float y) {
    out_all[(size_t)r * 2 * (size_t)frame + 2 * (size_t)s + ch] = y;
    render_append(ring, mask, RenderChannel{in, ch}, n0, s);
}

// {c0[t], dc[t]} of a voice whose taps an earlier launch left in global memory (fs_binaural_render.hip: the band FIR with an
// HRIR folded in), `folded` [taps], into s_cd.  In render_build_taps' place, under the same barriers.
__device__ __forceinline__ void render_load_taps(RenderTaps& s_cd, const float2* __restrict__ folded, int taps, int tid) {
    for (int t = tid; t < taps; t += kRenderTile) s_cd[t] = folded[t];
}

// ---- the voice bank (fs_internal.hpp: VoiceBankState, VoiceBankItem): the two passes of a callback whose rows are banks of voices.
// Unlike the pieces above each is a kernel's whole body, returns and barriers included.  What a renderer's voices carry beyond a
// delay and band gains — their aim — is the renderer's to say.

// The plan pass, one thread per (row, slot): reads the slot's device-resident state and the entry the host matched it with
// (Item::op), fixes what this callback ramps from and by how much in the slot's plan record, and writes the state the callback
// leaves behind; the thread of slot 0 also moves the row's sample counter on.  R, the renderer:
//   R::Aim                      what a voice aims at beyond its delay and band gains
//   R::read(v, set...)          ... of entry v (set: what the kernel passes through for it)
//   R::fade_out(st)             ... of an ending slot
//   R::from_silence(st, aim)    a starting slot's state: what it rises from
//   R::plan(pl, st, aim, it, slot)   the record's part of it: from st to aim
//   R::keep(st, aim)            the state's part of it after the callback
template <typename R, typename Item, typename Voice, typename Plan, typename... Set>
__device__ __forceinline__ void voice_bank_plan(const Item* __restrict__ items, const Voice* __restrict__ voices, Plan* __restrict__ plans,
                                                unsigned* __restrict__ n0_out, int count, int stride, int frame, int bands, float fs_f,
                                                Set... set) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = id / kVoiceSlots, slot = id % kVoiceSlots;
    if (r >= count) return;
    const Item& it = items[r];
    if (slot == 0) {
        const unsigned n0 = it.state->n0;
        n0_out[r] = n0;
        it.state->n0 = n0 + (unsigned)frame;
    }
    if (slot >= it.slots) return;
    const int op = it.op[slot];
    if (op == kVoiceIdle) return;
    auto st = it.state->slot[slot];
    Plan pl;
    float d1, g1[FS_MAX_BANDS];
    typename R::Aim aim;
    if (op == kVoiceEnd) {   // the delay freezes, the gains stay
        d1 = st.d0;
        for (int b = 0; b < FS_MAX_BANDS; ++b) g1[b] = st.g0[b];
        aim = R::fade_out(st);
    } else {
        const bool start = op >= kVoiceStart;
        const Voice v = voices[(size_t)r * (size_t)stride + (size_t)(start ? op - kVoiceStart : op - kVoiceContinue)];
        d1 = v.delay * fs_f;
        for (int b = 0; b < FS_MAX_BANDS; ++b) g1[b] = v.band_gain[b];
        aim = R::read(v, set...);
        if (start) {   // from its target, out of silence
            st.d0 = d1;
            for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = g1[b];
            R::from_silence(st, aim);
        }
        st.key = v.key;
    }
    const float e = render_slew(d1 - st.d0, frame);
    pl.d0 = st.d0;
    pl.e = e;
    for (int b = 0; b < FS_MAX_BANDS; ++b) { pl.g0[b] = st.g0[b]; pl.g1[b] = g1[b]; }
    R::plan(pl, st, aim, it, slot);
    plans[(size_t)r * kVoiceSlots + slot] = pl;
    if (op == kVoiceEnd) {
        st = decltype(st){};   // free
    } else {
        st.held = 1;
        st.d0 = pl.d0 + e;   // what the last output sample used: a == 1 there
        for (int b = 0; b < FS_MAX_BANDS; ++b) st.g0[b] = b < bands ? g1[b] : 0.0f;
        R::keep(st, aim);
    }
    it.state->slot[slot] = st;
}

// The render pass, a grid of (frame / kRenderTile output tiles) x 2 channels x rows.  A workgroup loops over its row's sounding
// slots in ascending order — the trip count and every branch around a barrier depend on the row only — and per slot puts the taps
// {c0[t], dc[t]} and the tile's read window into LDS (the window is per slot: every slot has a delay of its own), runs the
// four-accumulator tap loop of one output sample per thread and adds w * y to a register.  A thread past the frame's end keeps
// filling tables and windows and skips only the tap loop and the stores: nobody leaves before the last barrier.  After the last
// slot the thread stores its output and appends its input sample to the ring (render_store).  The renderer:
//   load_taps(s_cd, table, plp, ch, tid)   the slot's `taps` taps into s_cd (table: the row's band kernels), under render_build_taps' barriers
//   weight(plp, ch)                        {w0, dw} of the slot in channel ch
template <typename Item, typename Plan, typename LoadTaps, typename Weight>
__device__ __forceinline__ void voice_bank_render(const Item* __restrict__ items, const Plan* __restrict__ plans,
                                                  const unsigned* __restrict__ n0_all, const float* __restrict__ in_all,
                                                  float* __restrict__ out_all, int frame, int taps, LoadTaps&& load_taps, Weight&& weight) {
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
        if (ops[slot] == kVoiceIdle) continue;
        const Plan* __restrict__ plp = plans + (size_t)r * kVoiceSlots + slot;
        // (the scalars by value, the gain arrays through the record: indexing a copy by the band would put it in scratch)
        const float2 w0_dw = weight(plp, ch);
        struct { float d0, e, w0, dw; } pl = {plp->d0, plp->e, w0_dw.x, w0_dw.y};

        load_taps(s_cd, it.table, plp, ch, tid);
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
}  // namespace fs
