// fs_capi_publish.cpp — ReconstructImpulseResponse + the publish of its result (FSAC.cpp:320-380, GetImpulseResponse FSAC.h:113):
// the IR ring and its back-pressure, the three ways a ring slot becomes known as published (the compute stream's host word, a
// tail-stream batch's event, a slot's own event behind a copy), the reconstruct parts of a fused launch (owed_prepare /
// owed_publish), the stand-alone reconstruct on the tail stream (reconstruct_now) and the batched one (reconstruct_batch).
// Split out of fs_capi_frame.cpp in round 5; the frame pipeline that calls these lives in fs_capi_pipeline.cpp.
#include "fs_context.hpp"

namespace fsi {

// never overwrite the front buffer of the source's IR ring: at most kIrRing - 1 publishes in flight (publish seq reuses the
// slot of seq - kIrRing, so publish seq - kIrRing + 1 must have completed before seq is enqueued).  `more`: publishes about
// to be enqueued.  May block the host (the ring is the producer's only throttle) — call it without holding ir_mu.
int ir_ring_backpressure(fs_context* ctx, Source* s, int more) {
    poll_published(ctx, s);
    for (int j = 1; j <= more; ++j) {
        if (s->enqueued + (uint64_t)j < (uint64_t)kIrRing) continue;
        const uint64_t must = s->enqueued + (uint64_t)j + 1 - (uint64_t)kIrRing;
        const int slot = (int)(must % kIrRing);
        if (s->seq_of[slot] == must && s->front.load(std::memory_order_relaxed) < must) {
            FS_HIP(ctx, sync_publish(ctx, s, slot));
            poll_published(ctx, s);
        }
    }
    return FS_OK;
}

// publish number `seq` of the source has been enqueued: through the compute stream's host word (word != 0), a tail-stream
// batch's event (batch != 0) or the slot's own event.  (Readers look at enqueued, then seq_of, then the kind: written in reverse.)
// room: the publish carries FS_FLAG_ROOM_PARAMETERS records (fs_get_room_parameters)
static void note_publish(fs_context* ctx, Source* s, uint64_t seq, int slot, uint64_t batch = 0, uint64_t word = 0, bool room = false) {
    if (word) ctx->dbg.pub_word++; else ctx->dbg.pub_event++;
    s->room_of[slot] = room;
    s->pub_word[slot] = word; s->pub_batch[slot] = batch; s->seq_of[slot] = seq; s->enqueued = seq;
}

// FS_FLAG_ROOM_PARAMETERS: the source's [kIrRing][B] records and the context's parallel batch table, at the first flagged reconstruct
// (unflagged work allocates nothing)
int ensure_room(fs_context* ctx, Source* s) {
    if (!ctx->h_room_tab)
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_room_tab, sizeof(float*) * fs_context::kReconTabSlots * fs_context::kReconTabItems,
                                  hipHostMallocDefault));
    if (!s->h_room.load(std::memory_order_relaxed)) {
        fs_room_parameters* r = nullptr;
        const size_t bytes = sizeof(fs_room_parameters) * (size_t)kIrRing * (size_t)ctx->cfg.num_bands;
        FS_HIP(ctx, hipHostMalloc((void**)&r, bytes, hipHostMallocCoherent));
        std::memset(r, 0, bytes);
        s->h_room.store(r, std::memory_order_release);
    }
    return FS_OK;
}
static float* room_slot(const fs_context* ctx, const Source* s, int slot) {
    return reinterpret_cast<float*>(s->h_room.load(std::memory_order_relaxed) + (size_t)slot * (size_t)ctx->cfg.num_bands);
}

// before the COMPUTE stream writes the source's device IR set: whoever reads or writes it on the tail stream goes first
static hipError_t compute_waits_for_tail_ir(fs_context* ctx, Source* s) {
    if (s->cur_pub_seq) {
        const int slot = (int)(s->cur_pub_seq % kIrRing);
        if (s->seq_of[slot] == s->cur_pub_seq && !s->pub_word[slot]) {   // (a reused slot: that publish completed long ago)
            const uint64_t pb = s->pub_batch[slot];
            hipError_t e = hipSuccess;
            if (!pb) e = compute_waits_for(ctx, s->ev[slot]);
            else if (!tail_batch_done(ctx, pb)) e = hipStreamWaitEvent(ctx->stream, tail_batch_event(ctx, pb), 0);
            if (e != hipSuccess) return e;
        }
    }
    if (s->rev_recorded) return compute_waits_for(ctx, s->ev_rev);   // a reverb callback may be reading d_ir_mono
    return hipSuccess;
}

// a table slot of the batch kernel that its previous reader has certainly left
static int acquire_recon_tab(fs_context* ctx, unsigned* slot_out) {
    const unsigned slot_t = ctx->recon_tab_next++ % fs_context::kReconTabSlots;
    if (ctx->recon_tab_batch[slot_t] && !tail_batch_done(ctx, ctx->recon_tab_batch[slot_t]))
        FS_HIP(ctx, wait_event_polling(tail_batch_event(ctx, ctx->recon_tab_batch[slot_t])));
    if (ctx->recon_tab_word[slot_t] && !pub_word_done(ctx, ctx->recon_tab_word[slot_t])) FS_HIP(ctx, wait_pub_word(ctx, ctx->recon_tab_word[slot_t]));
    ctx->recon_tab_batch[slot_t] = 0; ctx->recon_tab_word[slot_t] = 0;
    *slot_out = slot_t;
    return FS_OK;
}

// ---- FS_FLAG_SPECTRAL_IR: the band carriers (definition: DESIGN.md section 8, "Spectral impulse responses") ----
static int carrier_log(const fs_context* ctx) {   // K = 2^n = the smallest power of two >= N
    int n = 0;
    while (n < 31 && (1ll << n) < (long long)ctx->num_samples) ++n;
    return n;
}
// bins [lo[b], lo[b+1]) of K/2 belong to band b: the first bin whose frequency k fs / K (double) reaches the band's lower edge
static bool band_bins(const fs_context* ctx, const double* inner, CarrierBands* out) {
    const int B = ctx->cfg.num_bands, n = carrier_log(ctx);
    const long long K = 1ll << n, half = K / 2;
    const double fs = (double)ctx->cfg.sample_rate;
    out->lo[0] = 1; out->lo[B] = (int32_t)half;
    for (int b = 1; b < B; ++b) {
        const double edge = inner[b - 1];
        if (!(edge > 0.0) || !(edge < fs / 2.0)) return false;
        long long k = (long long)std::ceil(edge * (double)K / fs);
        while (k > 0 && (double)(k - 1) * fs / (double)K >= edge) --k;
        while ((double)k * fs / (double)K < edge) ++k;
        out->lo[b] = (int32_t)std::min(std::max(k, 1ll), half);
    }
    for (int b = 0; b < B; ++b)
        if (out->lo[b + 1] <= out->lo[b]) return false;   // every band at least one bin (also: strictly ascending edges)
    return true;
}
static std::vector<double> effective_edges(const fs_context* ctx) {
    if (!ctx->band_edges.empty()) return ctx->band_edges;
    std::vector<double> e;
    for (int b = 1; b < ctx->cfg.num_bands; ++b) e.push_back(125.0 * std::pow(2.0, (double)b - 0.5));   // octave bands centred at 125, 250, ... Hz
    return e;
}

int check_band_edges(fs_context* ctx, const double* edges, const char* what) {
    if (carrier_log(ctx) > kCarrierMaxLog)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, std::string(what) + ": the carriers of " + std::to_string(ctx->num_samples) +
                                                      "-sample impulse responses exceed the largest FFT (2^24 points); fs_set_band_edges cannot change that");
    const std::vector<double> def = effective_edges(ctx);
    CarrierBands cb{};
    if (!band_bins(ctx, edges ? edges : def.data(), &cb))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, std::string(what) + ": every band edge must lie in (0, sample_rate / 2), ascending, and every "
                                                      "band must hold at least one FFT bin of " + std::to_string(ctx->cfg.sample_rate) + " / " +
                                                      std::to_string(1ll << carrier_log(ctx)) + " Hz" +
                                                      (edges || !ctx->band_edges.empty() ? std::string() :
                                                       std::string(" — the default octave edges do not fit this sample rate: give edges with fs_set_band_edges")));
    return FS_OK;
}

int check_spectral(fs_context* ctx, const fs_params* p) {
    if (!(p->flags & FS_FLAG_SPECTRAL_IR)) return FS_OK;
    return check_band_edges(ctx, nullptr, "FS_FLAG_SPECTRAL_IR");
}

std::vector<float2> host_twiddles(size_t N) {
    std::vector<float2> w(std::max<size_t>(N / 2, 1));
    for (size_t k = 0; k < N / 2; ++k) {
        const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)N;
        w[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    if (N < 2) w[0] = make_float2(1.f, 0.f);
    return w;
}

// The build of a carrier set of `rows` rows [rows][ld] through `work_rows` rows of complex work buffers: on the compute stream,
// waited for here (the work buffers are freed behind it).  launch(n, N, ld, bands, X, y, W, zeros, out) enqueues the set's passes
// (fs_fft.hip); what: whose build it is, for the messages; ms (or null): the device time of the passes.
template <class Launch>
static int build_carrier_set(fs_context* ctx, size_t rows, size_t work_rows, const char* what, const char* building, float** set, float* ms,
                             Launch launch) {
    *set = nullptr;
    const int n = carrier_log(ctx), N = ctx->num_samples, ld = carrier_stride(N);
    const size_t K = (size_t)1 << n;
    const std::vector<double> edges = effective_edges(ctx);
    CarrierBands bands{};
    if (!band_bins(ctx, edges.data(), &bands)) return check_band_edges(ctx, nullptr, what);
    const std::vector<float2> w = host_twiddles(K);
    float2 *X = nullptr, *y = nullptr, *W = nullptr;
    float *zeros = nullptr, *out = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipSetDevice(ctx->cfg.device);
    if (e == hipSuccess) e = hipMalloc((void**)&out, sizeof(float) * rows * (size_t)ld);
    if (e == hipSuccess) e = hipMalloc((void**)&X, sizeof(float2) * work_rows * K);
    if (e == hipSuccess) e = hipMalloc((void**)&y, sizeof(float2) * work_rows * K);
    if (e == hipSuccess) e = hipMalloc((void**)&W, sizeof(float2) * w.size());
    if (e == hipSuccess) e = hipMalloc((void**)&zeros, sizeof(float) * (K / 2 + 1));
    for (hipEvent_t& v : ev) if (ms && e == hipSuccess) e = hipEventCreate(&v);
    if (e == hipSuccess) e = hipMemcpyAsync(W, w.data(), sizeof(float2) * w.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(zeros, 0, sizeof(float) * (K / 2 + 1), ctx->stream);
    if (ms && e == hipSuccess) e = hipEventRecord(ev[0], ctx->stream);
    if (e == hipSuccess) {
        launch(n, N, ld, bands, X, y, W, zeros, out);
        e = hipGetLastError();
    }
    if (ms && e == hipSuccess) e = hipEventRecord(ev[1], ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (w is a local; the work buffers go next)
    if (ms && e == hipSuccess) e = hipEventElapsedTime(ms, ev[0], ev[1]);
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
    for (void* q : {(void*)X, (void*)y, (void*)W, (void*)zeros}) if (q) (void)hipFree(q);
    if (e != hipSuccess) {
        if (out) (void)hipFree(out);
        return ctx->hip_fail(e, (std::string(what) + ": building the " + building).c_str());
    }
    *set = out;
    return FS_OK;
}

// FS_FLAG_SPECTRAL_IR's B band carriers: once per context and band-edge setting
static int build_carriers(fs_context* ctx) {
    const size_t B = (size_t)ctx->cfg.num_bands;
    float ms = 0.0f;
    const int rc = build_carrier_set(ctx, B, B, "FS_FLAG_SPECTRAL_IR", "band carriers", &ctx->d_carrier, &ms,
                                     [&](int n, int N, int ld, const CarrierBands& bands, float2* X, float2* y, const float2* W, const float* zeros, float* out) {
                                         launch_build_carriers((int)B, n, N, ld, bands, X, y, W, zeros, out, ctx->stream);
                                     });
    if (rc == FS_OK) ctx->carrier_build_ms = ms;
    return rc;
}

// fs_reverb_ears_set: the 2B mid and side rows (fs_fft.hip: launch_build_ear_carriers)
int build_ear_carriers(fs_context* ctx, float radius_cm, float speed_cm_s, const char* what, float** set) {
    const size_t B = (size_t)ctx->cfg.num_bands;
    return build_carrier_set(ctx, 2 * B, 2 * B, what, "ear carriers", set, nullptr,
                             [&](int n, int N, int ld, const CarrierBands& bands, float2* X, float2* y, const float2* W, const float* zeros, float* out) {
                                 launch_build_ear_carriers((int)B, n, N, ld, bands, (double)ctx->cfg.sample_rate, (double)radius_cm, (double)speed_cm_s,
                                                           X, y, W, zeros, out, ctx->stream);
                             });
}

// fs_reverb_soundfield_set: C channels of B rows (fs_fft.hip: launch_build_soundfield_carriers); the work buffers are those of
// one channel
int build_soundfield_carriers(fs_context* ctx, int32_t order, const char* what, float** set) {
    const int C = (order + 1) * (order + 1);
    const size_t B = (size_t)ctx->cfg.num_bands;
    return build_carrier_set(ctx, (size_t)C * B, B, what, "soundfield carriers", set, nullptr,
                             [&](int n, int N, int ld, const CarrierBands& bands, float2* X, float2* y, const float2* W, const float* zeros, float* out) {
                                 launch_build_soundfield_carriers(C, (int)B, n, N, ld, bands, X, y, W, zeros, out, ctx->stream);
                             });
}

// The installation of an ear or soundfield set in place of the one in force (*slot; set == nullptr: none), behind the reverb stream
static int install_carrier_set(fs_context* ctx, float** slot, uint64_t* gen, float* set, const char* what) {
    hipError_t e = hipStreamSynchronize(ctx->rev_stream);   // (no callback's launches still read the set in force)
    if (e == hipSuccess && *slot) e = hipFree(*slot);
    if (e != hipSuccess) {   // (the set in force stays; the new one is not kept)
        if (set) (void)hipFree(set);
        return ctx->hip_fail(e, what);
    }
    *slot = set;
    ++*gen;
    return FS_OK;
}

int install_ear_carriers(fs_context* ctx, float* set, float radius_cm, float speed_cm_s) {
    const int rc = install_carrier_set(ctx, &ctx->d_ear_carrier, &ctx->ear_set_gen, set, "installing the ear carriers");
    if (rc) return rc;
    ctx->ear_radius_cm = set ? radius_cm : 0.0f;
    ctx->ear_speed_cm_s = set ? speed_cm_s : 0.0f;
    return FS_OK;
}

int install_soundfield_carriers(fs_context* ctx, float* set, int32_t order) {
    const int rc = install_carrier_set(ctx, &ctx->d_sf_carrier, &ctx->sf_set_gen, set, "installing the soundfield carriers");
    if (rc) return rc;
    ctx->sf_order = set ? order : -1;
    return FS_OK;
}

int carrier_for(fs_context* ctx, const fs_params* p, const float** out) {
    *out = nullptr;
    if (!(p->flags & FS_FLAG_SPECTRAL_IR)) return FS_OK;
    if (!ctx->d_carrier) { const int rc = build_carriers(ctx); if (rc) return rc; }
    *out = ctx->d_carrier;
    return FS_OK;
}

static int spb_of(const fs_context* ctx, const fs_params& p) {
    return p.samples_per_bin > 0 ? p.samples_per_bin : (int)std::ceil(ctx->cfg.bin_duration * (float)ctx->cfg.sample_rate);   // FSAC.cpp:324
}

int owed_prepare(fs_context* ctx, FrameParts& fp, OwedLaunch& ol) {
    if (ctx->recon_owed.empty()) return FS_OK;
    size_t take = 0;   // the oldest entries that are due (frame order: a prefix); summed entries wait one launch (ReconOwed::reduced)
    while (take < ctx->recon_owed.size() && take < (size_t)kMaxReconParts &&
           (!ctx->recon_owed[take].reduced || ctx->recon_owed[take].age >= 1)) ++take;
    for (size_t k = take; k < ctx->recon_owed.size(); ++k) ctx->recon_owed[k].age++;
    if (take == 0) return FS_OK;
    // (the entries leave recon_owed only when everything that can fail here has succeeded: on an error they are still owed
    // and the next flush reconstructs them)
    ol.owed.assign(ctx->recon_owed.begin(), ctx->recon_owed.begin() + (long)take);
    const int B = ctx->cfg.num_bands;
    std::vector<Source*> distinct;
    for (const fs_context::ReconOwed& o : ol.owed)
        if (std::find(distinct.begin(), distinct.end(), o.s) == distinct.end()) distinct.push_back(o.s);
    std::sort(distinct.begin(), distinct.end());           // one locking order for every thread
    // the ring's back-pressure and the table slot BEFORE the IR mutexes are taken: both may wait for the GPU, and
    // fs_reverb_process on the audio thread must never queue behind such a wait
    for (Source* s : distinct) {
        int more = 0;
        for (const fs_context::ReconOwed& o : ol.owed) more += o.s == s ? 1 : 0;
        const int br = ir_ring_backpressure(ctx, s, more);
        if (br) { ol.owed.clear(); return br; }
    }
    const float* carrier = nullptr;   // (built before any mutex is taken: the first build waits for the GPU)
    for (const fs_context::ReconOwed& o : ol.owed) {
        if (carrier || !(o.p.flags & FS_FLAG_SPECTRAL_IR)) continue;
        const int cr = carrier_for(ctx, &o.p, &carrier);
        if (cr) { ol.owed.clear(); return cr; }
    }
    { const int ar = acquire_recon_tab(ctx, &ol.tab_slot); if (ar) { ol.owed.clear(); return ar; } }
    ReconItem* tab = ctx->h_recon_tab + (size_t)ol.tab_slot * fs_context::kReconTabItems;
    auto bail = [&](int rc) { ol.owed.clear(); ol.seq.clear(); ol.newest.clear(); ol.locks.clear(); fp.num_recon = 0; return rc; };
#define FS_OWED_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bail(ctx->hip_fail(e_, #call)); } while (0)
    for (Source* s : distinct) ol.locks.emplace_back(s->ir_mu);
    fp.num_recon = 0; fp.recon_tab = tab; fp.recon_B = B; fp.recon_nb = ctx->num_bins; fp.recon_samples = ctx->num_samples;
    fp.recon_carrier = carrier;   // (nullptr unless some item is spectral)
    ol.pub = next_pub_word(ctx);
    fp.pub = ol.pub;
    for (size_t i = 0; i < ol.owed.size(); ++i) {
        const fs_context::ReconOwed& o = ol.owed[i];
        Source* s = o.s;
        bool later = false;                                // a later frame of the same source in this launch?
        for (size_t k = i + 1; k < ol.owed.size(); ++k) later = later || ol.owed[k].s == s;
        uint64_t seq = s->enqueued + 1;                    // (the ring's back-pressure was applied above, before the mutexes)
        for (size_t k = 0; k < i; ++k) seq += ol.owed[k].s == s ? 1 : 0;
        const int slot = (int)(seq % kIrRing);
        // An IR that is superseded within the launch only goes to its ring slot (the channel row); the source's newest IR of the
        // launch also becomes the device-resident set (the reverb's, fs_copy_band_impulse_response's).
        if (!later) FS_OWED_HIP(compute_waits_for_tail_ir(ctx, s));
        if (o.reduced && s->red_recorded[o.cur]) FS_OWED_HIP(compute_waits_for(ctx, s->ev_red[o.cur]));   // the sum over the ranks (done a launch ago)
        ol.seq.push_back(seq); ol.newest.push_back(later ? 0 : 1);
        ReconItem& r = tab[fp.num_recon++];
        r.energy = s->d_energy[o.cur]; r.ir_bands = later ? nullptr : s->d_ir_bands; r.ir_mono = later ? nullptr : s->d_ir_mono;
        r.host = s->h_ir[slot]; r.mask = slot_mask_ptr(ctx, s, slot); r.spb = spb_of(ctx, o.p);
        r.spectral = (o.p.flags & FS_FLAG_SPECTRAL_IR) ? 1 : 0;
    }
#undef FS_OWED_HIP
    ctx->recon_owed.erase(ctx->recon_owed.begin(), ctx->recon_owed.begin() + (long)take);
    return FS_OK;
}
// behind the launch: note the publishes (the launch announces them itself); a source with a reverb also gets an event on the
// compute stream for its callbacks to wait on
int owed_publish(fs_context* ctx, OwedLaunch& ol, bool launched_fused) {
    if (ol.owed.empty()) return FS_OK;
    const int B = ctx->cfg.num_bands;
    if (!launched_fused) {   // no fused form for this launch: the same table through the batch kernel, on the compute stream
        launch_reconstruct_batch(ctx->h_recon_tab + (size_t)ol.tab_slot * fs_context::kReconTabItems, (int)ol.owed.size(), B, ctx->num_bins,
                                 ctx->num_samples, ctx->stream, ol.pub, ctx->d_carrier);
        FS_HIP(ctx, hipGetLastError());
    }
    ctx->recon_tab_word[ol.tab_slot] = ol.pub.id;          // the slot's reader: this launch
    ctx->pub_issued = ol.pub.id;
    for (size_t i = 0; i < ol.owed.size(); ++i) {
        const fs_context::ReconOwed& o = ol.owed[i];
        Source* s = o.s;
        s->rec_recorded[o.cur] = true; s->rec_on_compute[o.cur] = true; s->rec_batch[o.cur] = 0;
        if (ol.newest[i]) {   // (ir_mu is held)
            s->last_rec = o.cur; s->cur_pub_seq = 0; s->dev_ir_word = ol.pub.id; s->ir_gen++;
            if (s->d_ring) FS_HIP(ctx, hipEventRecord(s->ev_rec[o.cur], ctx->stream));   // fs_reverb_process reads d_ir_mono behind this
        }
        note_publish(ctx, s, ol.seq[i], (int)(ol.seq[i] % kIrRing), 0, ol.pub.id);
    }
    ol.locks.clear();
    return FS_OK;
}

// the reconstructs that were waiting for the next fused launch, on the tail stream after all (a flush, or a reconstruct
// that must not overtake them)
int run_owed_reconstructs(fs_context* ctx) {
    if (ctx->recon_owed.empty()) return FS_OK;
    std::vector<fs_context::ReconOwed> owed;
    owed.swap(ctx->recon_owed);
    ctx->dbg.owed_on_tail += owed.size();
    for (const fs_context::ReconOwed& o : owed) {
        // (tail_ordered = o.reduced: the tail stream is behind the all-reduce, which is behind the launch)
        const SourceFrameScope frame(o.s, o.cur, o.fixed, o.reduced, /*tail_ordered=*/o.reduced, /*keep_if_current=*/false);
        const int rc = flush_reconstruct(ctx, o.s, &o.p);
        if (rc) return rc;
    }
    return FS_OK;
}

// A reconstruct that no launch is fused with (a flush: fs_submit, fs_synchronize, an observer): on one GPU it goes onto the
// COMPUTE stream as a batch of one — the kernel writes the published host slot itself, nothing crosses to the tail stream.
// (Through the tail stream — a handoff event, a kernel and a copy on the priority queue while the compute queue is busy — one
// flush in three took 6 ms longer than the others on the pool's boxes: tools/repeat_driver_bench.py, the driver's 20-step
// region read 440 or 880 M rays/s.)
int flush_reconstruct(fs_context* ctx, Source* s, const fs_params* p) {
    if (!ctx->comm && ctx->cfg.world_size == 1) { Source* one = s; return reconstruct_batch(ctx, &one, 1, p, true); }
    return reconstruct_now(ctx, s, p);
}

int reconstruct_now(fs_context* ctx, Source* s, const fs_params* p) {
    { const int orc = run_owed_reconstructs(ctx); if (orc) return orc; }   // IRs are published in frame order
    // ReconstructImpulseResponse is not linear in the energy (a = e / sqrt(e * Pi4)): the IR of a rank's PARTIAL
    // histogram is not a partial IR.  A sharded context only reconstructs a frame that was summed over the ranks — by
    // the library (fs_comm_init / fs_comm_attach) or by the caller's collective on the tail stream (fs_energy_handoff).
    if (ctx->cfg.world_size > 1 && !s->reduced && !s->handed_off)
        return ctx->fail(FS_ERR_COMM, "world_size > 1: the energy buffer holds this rank's partial sums only — attach a "
                                      "communicator (fs_comm_init) or reduce it behind fs_energy_handoff before reconstructing");
    const float* carrier = nullptr;
    { const int cr = carrier_for(ctx, p, &carrier); if (cr) return cr; }
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const int B = ctx->cfg.num_bands;
    int spb = p->samples_per_bin > 0 ? p->samples_per_bin
                                     : (int)std::ceil(ctx->cfg.bin_duration * (float)ctx->cfg.sample_rate);  // FSAC.cpp:324

    { const int br = ir_ring_backpressure(ctx, s, 1); if (br) return br; }
    const bool room = (p->flags & FS_FLAG_ROOM_PARAMETERS) != 0;
    if (room) { const int rr = ensure_room(ctx, s); if (rr) return rr; }
    TimedFrame tf{};
    bool timed = ctx->profiling >= 2;
    if (timed) {
        for (int i = 0; i < 5; ++i) tf.e[i] = nullptr;
        tf.e[3] = take_event(ctx);
        tf.e[4] = take_event(ctx);
    }
    if (p->flags & FS_FLAG_FLUSH_BEFORE_RECONSTRUCT) {  // ARTS.cpp:191 literally
        FS_HIP(ctx, wait_energy_readers(ctx, s));
        FS_HIP(ctx, hipMemsetAsync(s->energy(), 0, sizeof(float) * (size_t)B * (size_t)ctx->num_bins, ctx->stream));
        // (deterministic mode: the fp32 buffer is re-derived from the fixed-point histogram below — the flush empties that one too)
        if (s->cur_fixed && s->d_fixed[s->cur])
            FS_HIP(ctx, hipMemsetAsync(s->d_fixed[s->cur], 0, sizeof(unsigned long long) * (size_t)B * (size_t)ctx->num_bins, ctx->stream));
    }
    // The tail stream takes over: it waits for this frame's deposit (and runs behind any collective the caller
    // put there after fs_energy_handoff), reconstructs and publishes while the compute stream goes on to the
    // next frame.  Reconstructs and publishes of one source are ordered among themselves by the tail stream.
    // (A frame the library has just summed over the ranks — or that the caller took over with fs_energy_handoff — is
    // already ordered: a second event pair per frame on the compute stream is a second bubble between its launches,
    // 2 % of a cfg3 frame: tools/rccl_tax.sh.)
    if (!s->tail_ordered || (p->flags & FS_FLAG_FLUSH_BEFORE_RECONSTRUCT)) FS_HIP(ctx, handoff_energy(ctx, s));
    else FS_HIP(ctx, tail_waits_for_compute_ir(ctx, s));   // (a fused reconstruct of an earlier frame may still be writing d_ir_*)
    hipStream_t tail = ctx->copy_stream;
    {
        std::lock_guard<std::mutex> g(s->ir_mu);   // against fs_reverb_process on the audio thread
        if (s->rev_recorded) FS_HIP(ctx, hipStreamWaitEvent(tail, s->ev_rev, 0));   // a reverb callback may be reading d_ir_mono
        if (timed) FS_HIP(ctx, hipEventRecord(tf.e[3], tail));
        // deterministic mode: the collective summed the fixed-point histogram; round it to fp32 once, now
        if (s->cur_fixed && !s->reduced) launch_fixed_to_energy(s->d_fixed[s->cur], s->energy(), B * ctx->num_bins, tail);
        launch_reconstruct(s->energy(), B, ctx->num_bins, ctx->cfg.sample_rate, ctx->num_samples, spb, s->d_ir_bands,
                           s->d_ir_mono, tail, carrier);
        FS_HIP(ctx, hipGetLastError());
        FS_HIP(ctx, hipEventRecord(s->ev_rec[s->cur], tail));
        s->rec_recorded[s->cur] = true; s->rec_batch[s->cur] = 0; s->rec_on_compute[s->cur] = false;
        s->last_rec = s->cur; s->ir_gen++;
    }
    uint64_t seq = s->enqueued + 1;
    int slot = (int)(seq % kIrRing);
    if (room) {   // the records go into the slot before its event is recorded (the same histogram the reconstruct read)
        launch_room_parameters(s->energy(), B, ctx->num_bins, ctx->cfg.bin_duration, room_slot(ctx, s, slot), tail);
        FS_HIP(ctx, hipGetLastError());
    }
    FS_HIP(ctx, hipMemcpyAsync(s->h_ir[slot], s->d_ir_mono, sizeof(float) * (size_t)ctx->num_samples,
                               hipMemcpyDeviceToHost, tail));
    FS_HIP(ctx, slot_mask_all_dirty(ctx, s, slot, tail));   // (a copy wrote every block: the kernels' zero-block bookkeeping starts over)
    FS_HIP(ctx, hipEventRecord(s->ev[slot], tail));
    note_publish(ctx, s, seq, slot, 0, 0, room);
    s->cur_pub_seq = seq; s->dev_ir_word = 0;
    ctx->dbg.tail_ops += 4;   // the reconstruct kernel, its event, the copy, the publish event
    if (timed) {
        FS_HIP(ctx, hipEventRecord(tf.e[4], tail));
        tf.has_recon = true;
        ctx->pending.push_back(tf);
    }
    return FS_OK;
}

int ir_ring_backpressure_for(fs_context* ctx, Source* s) { return ir_ring_backpressure(ctx, s, 1); }

// Before the TAIL stream writes the source's device IR set: the compute-stream launch that wrote it last (a fused reconstruct part,
// a batch behind a tick) may still be running — the compute stream hands over (everything it has enqueued so far goes first).
hipError_t tail_waits_for_compute_ir(fs_context* ctx, Source* s) {
    if (!s->dev_ir_word || pub_word_done(ctx, s->dev_ir_word)) return hipSuccess;
    hipError_t e = hipEventRecord(s->ev_dep, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_stream, s->ev_dep, 0);
    ctx->dbg.tail_ops++;
    return e;
}

// ReconstructImpulseResponse + publish of MANY sources' current frames (the subsystem's loop over ActiveSources,
// ARTS.cpp:100-126, every one ending in ReconstructImpulseResponse :192): one handoff, ONE kernel that also writes the
// channel views straight into the sources' pinned host ring slots, ONE event — instead of a wait, a kernel, a copy and
// three event records per source (67 us per source of host and queue time: 128 sources took 8.6 ms, 32 took 2.8).
// Anything unusual about a source's frame (a literal second flush, per-kernel timing) sends the whole batch the ordinary way.
// on_compute (fs_update_sources: the caller waits for the tick anyway): the launch goes onto the COMPUTE stream, right behind
// the frame's connect pass — no event pair, no second stream to wake (12 us between the two kernels of a one-source tick).
int reconstruct_batch(fs_context* ctx, Source* const* srcs, int count, const fs_params* p, bool on_compute) {
    { const int orc = run_owed_reconstructs(ctx); if (orc) return orc; }   // IRs are published in frame order
    bool plain = ctx->profiling < 2 && !(p->flags & FS_FLAG_FLUSH_BEFORE_RECONSTRUCT);   // (also for ONE source: no copy command, one event)
    for (int i = 0; i < count; ++i)
        if (ctx->cfg.world_size > 1 && !srcs[i]->reduced && !srcs[i]->handed_off) plain = false;   // (reconstruct_now refuses with the message)
    if (!plain) {
        for (int i = 0; i < count; ++i) { const int rc = reconstruct_now(ctx, srcs[i], p); if (rc) return rc; }
        return FS_OK;
    }
    const float* carrier = nullptr;
    { const int cr = carrier_for(ctx, p, &carrier); if (cr) return cr; }
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const int B = ctx->cfg.num_bands;
    const int spb = p->samples_per_bin > 0 ? p->samples_per_bin : (int)std::ceil(ctx->cfg.bin_duration * (float)ctx->cfg.sample_rate);  // FSAC.cpp:324
    hipStream_t tail = on_compute ? ctx->stream : ctx->copy_stream;
    const bool room = (p->flags & FS_FLAG_ROOM_PARAMETERS) != 0;
    for (int first = 0; first < count; first += fs_context::kReconTabItems) {
        const int n = std::min(count - first, (int)fs_context::kReconTabItems);
        Source* const* g = srcs + first;
        for (int i = 0; i < n; ++i) { const int br = ir_ring_backpressure(ctx, g[i], 1); if (br) return br; }   // (before the mutexes: may wait for the GPU)
        for (int i = 0; i < n && room; ++i) { const int rr = ensure_room(ctx, g[i]); if (rr) return rr; }
        // the tail stream takes over behind everything the compute stream has enqueued for these frames: one event pair
        bool ordered = true;   // (on_compute: the compute stream is behind its own kernels)
        for (int i = 0; i < n && !on_compute; ++i)
            ordered = ordered && g[i]->tail_ordered && (!g[i]->dev_ir_word || pub_word_done(ctx, g[i]->dev_ir_word));
        if (!ordered) {
            FS_HIP(ctx, handoff_energy(ctx, g[0]));
            for (int i = 0; i < n; ++i) g[i]->tail_ordered = true;
        }
        unsigned slot_t = 0;
        { const int ar = acquire_recon_tab(ctx, &slot_t); if (ar) return ar; }
        ReconItem* tab = ctx->h_recon_tab + (size_t)slot_t * fs_context::kReconTabItems;
        float** room_tab = room ? ctx->h_room_tab + (size_t)slot_t * fs_context::kReconTabItems : nullptr;   // (read by the same launch as tab)
        std::vector<Source*> order(g, g + n);
        std::sort(order.begin(), order.end());                 // one locking order for every thread
        std::vector<std::unique_lock<std::mutex>> locks;
        locks.reserve((size_t)n);
        for (Source* s : order) locks.emplace_back(s->ir_mu);  // against fs_reverb_process on the audio thread
        // on the tail stream: ONE event for the batch (tail_batch_ev; the ids are totally ordered because only the tail stream
        // issues them); on the compute stream: the launch announces itself in the host word (publish_arrive)
        const uint64_t batch = on_compute ? 0 : ctx->tail_batch_newest.load(std::memory_order_relaxed) + 1;
        const PublishWord pub = on_compute ? next_pub_word(ctx) : PublishWord();
        for (int i = 0; i < n; ++i) {
            Source* s = g[i];
            if (on_compute) FS_HIP(ctx, compute_waits_for_tail_ir(ctx, s));   // nor write d_ir_* under a publish the tail stream still copies from
            else if (s->rev_recorded) FS_HIP(ctx, hipStreamWaitEvent(tail, s->ev_rev, 0));   // a reverb callback may be reading d_ir_mono
            // deterministic mode: the collective summed the fixed-point histogram; round it to fp32 once, now
            if (s->cur_fixed && !s->reduced) launch_fixed_to_energy(s->d_fixed[s->cur], s->energy(), B * ctx->num_bins, tail);
            const uint64_t seq = s->enqueued + 1;
            const int slot = (int)(seq % kIrRing);
            tab[i].energy = s->energy(); tab[i].ir_bands = s->d_ir_bands; tab[i].ir_mono = s->d_ir_mono; tab[i].host = s->h_ir[slot];
            tab[i].mask = slot_mask_ptr(ctx, s, slot);
            tab[i].spb = spb; tab[i].spectral = carrier != nullptr ? 1 : 0;
            if (room_tab) room_tab[i] = room_slot(ctx, s, slot);
        }
        launch_reconstruct_batch(tab, n, B, ctx->num_bins, ctx->num_samples, tail, pub, carrier, room_tab, ctx->cfg.bin_duration);
        FS_HIP(ctx, hipGetLastError());
        if (on_compute) {
            ctx->pub_issued = pub.id;
            ctx->recon_tab_word[slot_t] = pub.id;
        } else {
            FS_HIP(ctx, hipEventRecord(ctx->tail_batch_ev[batch % fs_context::kTailBatches], tail));
            ctx->dbg.tail_ops += 2;
            ctx->tail_batch_newest.store(batch, std::memory_order_release);
            ctx->recon_tab_batch[slot_t] = batch;
        }
        for (int i = 0; i < n; ++i) {
            Source* s = g[i];
            s->rec_recorded[s->cur] = true; s->rec_batch[s->cur] = batch; s->rec_on_compute[s->cur] = on_compute;
            s->last_rec = s->cur; s->ir_gen++;
            const uint64_t seq = s->enqueued + 1;
            note_publish(ctx, s, seq, (int)(seq % kIrRing), batch, pub.id, room);
            if (on_compute) {
                s->cur_pub_seq = 0; s->dev_ir_word = pub.id;
                if (s->d_ring) FS_HIP(ctx, hipEventRecord(s->ev_rec[s->cur], ctx->stream));   // fs_reverb_process reads d_ir_mono behind this
            } else {
                s->cur_pub_seq = seq; s->dev_ir_word = 0;
            }
        }
    }
    return FS_OK;
}

}  // namespace fsi
