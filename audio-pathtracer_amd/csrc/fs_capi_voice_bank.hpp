// fs_capi_voice_bank.hpp — the callback of a renderer whose sources hold a voice bank (fs_reflection_render_process_batch,
// fs_binaural_render_process_batch, fs_ambisonic_render_process_batch), from its arguments to the caller's arrays: everything validated, the voices matched to the
// slots on the host's copy of the slot table (voice_match), one copy up, the renderer's launches, one copy back, one wait.  What a
// renderer is beyond that arrives as a descriptor and four callables.  Host code only; the bank's other half — the matching, the
// inits and the releases — is fs_capi_reflect_render.cpp's, the device's fs_dev_render.hpp's.
#pragma once

#include <array>
#include <type_traits>

#include "fs_context.hpp"

namespace fsi {

// What one of the three renderers is, beyond its kernels: its bank on a source, its staging, its messages (no_set: the refusal
// while no HRIR set is in force; nullptr: it needs none), its launches and the bytes of its bank's header, behind which the
// history begins.
template <typename Batch>
struct VoiceBankRenderer {
    VoiceBank Source::*bank;
    CallbackStage fs_context::*stage;
    const char *no_setup, *no_set;
    void (*launch)(const Batch&, hipStream_t);
    size_t header;
};

// A voice-bank callback, every check in the order the header gives.
//   entry_ok(v)      an entry's own fields, behind its key, delay and band gains: FS_OK, or the failure reported
//   row_ok(bank)     a row's own check, between its first checks (render_row) and its voice count: likewise
//   extra(slots, shape)   {up, scratch, row}: the bytes of the renderer's own upload and scratch block (CallbackLayout::up[kOwn]
//                    and ::scratch[kOwn]; 0: none) and the floats of an output row, slots = the sum of the rows' slot counts,
//                    shape = the set-up the rows share
//   fill(b, items, h_up, d_up, d_scratch)   what the launches read beyond the bank's part of b, and what goes up in the renderer's
//                    own block: called with the items filled (items: the host's) and before the copy up; the three pointers
//                    are the own blocks — the upload's two sides and the scratch
template <typename Batch, typename Voice, typename Row, typename EntryOk, typename RowOk, typename Extra, typename Fill>
int voice_bank_process(const VoiceBankRenderer<Batch>& q, fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                       const Voice* voices, const int32_t* voice_counts, int32_t stride, float* out, float* mix, Row* rows, EntryOk&& entry_ok,
                       RowOk&& row_ok, Extra&& extra, Fill&& fill) {
    using Item = std::remove_const_t<std::remove_pointer_t<decltype(Batch::items)>>;
    using Plan = std::remove_pointer_t<decltype(Batch::plans)>;
    if (!ctx || !sources || !in || !voices || !voice_counts || (!out && !mix)) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (count < 1 || count > FS_MAX_REFLECTION_RENDER_BATCH)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REFLECTION_RENDER_BATCH)");
    if (stride < 1 || stride > FS_MAX_REFLECTION_VOICES)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "stride out of range (1 .. FS_MAX_REFLECTION_VOICES)");
    if (q.no_set && ctx->hrtf_dirs == 0) return ctx->fail(FS_ERR_INVALID_ARGUMENT, q.no_set);
    // Everything is validated before the first state change or enqueue: a refused call changes nothing.
    auto setup_of = [&](const Source& s) -> const RenderSetup& { return (s.*q.bank).r; };
    std::vector<Source*> srcs((size_t)count);
    size_t slots_total = 0;
    for (int32_t i = 0; i < count; ++i) {
        int rc;
        Source* s = srcs[(size_t)i] = render_row(ctx, sources[i], setup_of, q.no_setup, i ? srcs[0] : nullptr, &rc);
        if (rc) return rc;
        const VoiceBank& bank = s->*q.bank;
        rc = row_ok(bank);
        if (rc) return rc;
        slots_total += (size_t)bank.voices;
        const int32_t n = voice_counts[i];
        if (n < 0 || n > stride) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a voice count outside 0 .. stride");
        const Voice* v = voices + (size_t)i * (size_t)stride;
        for (int32_t e = 0; e < n; ++e) {
            for (int32_t f = 0; f < e; ++f)
                if (v[f].key == v[e].key) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a key appears twice in one row");
            rc = render_aim_check(ctx, "voice", v[e].delay, v[e].band_gain, bank.r);
            if (!rc) rc = entry_ok(v[e]);
            if (rc) return rc;
        }
    }
    { const int rc = render_no_duplicates(ctx, srcs); if (rc) return rc; }
    const RenderSetup& shape = setup_of(*srcs[0]);
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    enum { kItems, kVoices, kOwn, kN0 = 0, kPlans };   // CallbackLayout::up and ::scratch (kOwn: of both)
    const size_t voices_bytes = sizeof(Voice) * (size_t)count * (size_t)stride;
    const std::array<size_t, 3> own = extra(slots_total, shape);
    const CallbackLayout l = callback_layout(count, shape.frame, own[2], {sizeof(Item) * (size_t)count, voices_bytes, own[0]},
                                             {sizeof(unsigned) * (size_t)count, sizeof(Plan) * (size_t)count * kVoiceSlots, own[1]});
    CallbackStage& st = ctx->*q.stage;
    { const int rc = st.fit(ctx, l.host_bytes, l.dev_bytes); if (rc) return rc; }
    char* hs = st.h; char* ds = st.d;
    Item* items = (Item*)(hs + l.up[kItems]);
    std::vector<VoiceMatch> matches((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        const VoiceBank& bank = srcs[(size_t)i]->*q.bank;
        const VoiceMatch& m = matches[(size_t)i] = voice_match(bank, voices + (size_t)i * (size_t)stride, sizeof(Voice), voice_counts[i]);
        Item& it = items[i];
        std::memset(&it, 0, sizeof(it));
        it.state = (decltype(it.state))bank.r.d;
        it.ring = (float*)(bank.r.d + q.header);
        it.table = bank.r.table;
        it.mask = bank.r.ring - 1u;
        it.slots = bank.voices;
        std::memcpy(it.op, m.op, sizeof(it.op));
    }
    std::memcpy(hs + l.up[kVoices], voices, voices_bytes);
    std::memcpy(hs + l.in, in, l.in_rows);
    Batch b{};
    b.items = (const Item*)(ds + l.up[kItems]);
    b.voices = (const Voice*)(ds + l.up[kVoices]);
    b.plans = (Plan*)(ds + l.scratch[kPlans]);
    b.n0 = (unsigned*)(ds + l.scratch[kN0]);
    b.count = count; b.stride = stride; b.frame = shape.frame; b.taps = shape.taps; b.bands = ctx->cfg.num_bands;
    b.fs = (float)ctx->cfg.sample_rate;
    b.in = (const float*)(ds + l.in);
    b.out = (float*)(ds + l.d_out);
    b.mix = mix ? (float*)(ds + l.d_mix) : nullptr;
    fill(b, items, hs + l.up[kOwn], ds + l.up[kOwn], ds + l.scratch[kOwn]);
    FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
    q.launch(b, rs);
    FS_HIP(ctx, hipGetLastError());
    for (int32_t i = 0; i < count; ++i) {   // the plan pass is on its way: the slot tables are what it leaves behind
        VoiceBank& bank = srcs[(size_t)i]->*q.bank;
        std::memcpy(bank.held, matches[(size_t)i].held, sizeof(bank.held));
        std::memcpy(bank.key, matches[(size_t)i].key, sizeof(bank.key));
    }
    { const int rc = callback_finish(ctx, st, l, out != nullptr, mix); if (rc) return rc; }
    if (out) std::memcpy(out, hs + l.h_out, l.rows);
    if (rows)
        for (int32_t i = 0; i < count; ++i) {
            const fs_reflection_render_row& r = matches[(size_t)i].row;
            rows[i] = Row{r.sounding, r.started, r.ended, r.dropped};
        }
    return FS_OK;
}

}  // namespace fsi
