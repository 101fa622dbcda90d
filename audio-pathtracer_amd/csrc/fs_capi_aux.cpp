// fs_capi_aux.cpp — rows beside the core path: legacy forward tracer (a9), the engine line trace (tests / tools),
// text interchange (f1), reverb convolution (f2), frequency-domain material response (f4).
#include "fs_context.hpp"

extern "C" {

// ---- legacy forward tracer (a9) -----------------------------------------------------------------------------
void fs_sound_params_default(fs_sound_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(fs_sound_params);
    p->seed = 0x5EEDull;
    p->raycasts_per_tick = 1500;   // FSAC.h:39
    p->raycast_bounces = 10;       // FSAC.h:42
    p->raycast_distance = 5000.f;  // FSAC.h:45
    p->simulated_duration = 1.0f;  // FSAC.h:136
    p->listener_radius = 34.0f;    // ADefaultPawn collision sphere (engine default, build-owned)
}

// rays per wave of the tracer, the other lanes help (64 = no sharing; 2 vs 4: 0.259 vs 0.267 ms at 100 k triangles, 0.195 vs 0.212 at 5 k)
constexpr int kSoundRaysPerWave = 2;

int fs_update_sound(fs_context* ctx, fs_source h, const fs_sound_params* p, fs_sound_result* out) {
    if (!ctx || !out) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    { int ir = maybe_install_refined(ctx); if (ir) return ir; }                     // fs_scene_commit_progressive: the better tree is ready
    if (ctx->refit_pending) { int rr = fs_scene_refit(ctx); if (rr) return rr; }   // moved triangles: refit before tracing
    fs_sound_params def;
    if (!p) { fs_sound_params_default(&def); p = &def; }
    if (p->struct_size != sizeof(fs_sound_params)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_sound_params.struct_size mismatch");
    if (p->raycasts_per_tick < 0 || p->raycast_bounces < 0 || !(p->listener_radius >= 0.f))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad sound params");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (!ctx->d_sound) FS_HIP(ctx, hipMalloc((void**)&ctx->d_sound, sizeof(SoundAccum)));
    SoundKParams sp{};
    sp.seed_lo = (uint32_t)p->seed;
    sp.seed_hi = (uint32_t)(p->seed >> 32);
    sp.raycasts_per_tick = p->raycasts_per_tick;
    sp.raycast_bounces = p->raycast_bounces;
    sp.raycast_distance = p->raycast_distance;
    sp.simulated_duration = p->simulated_duration;
    sp.listener_radius = p->listener_radius;
    std::memcpy(sp.src, s->pos, sizeof(sp.src));
    std::memcpy(sp.lis, ctx->listener, sizeof(sp.lis));
    FS_HIP(ctx, hipMemsetAsync(ctx->d_sound, 0, sizeof(SoundAccum), ctx->stream));
    launch_update_sound(ctx->scene, sp, ctx->d_sound, kSoundRaysPerWave, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    SoundAccum acc{};
    FS_HIP(ctx, hipMemcpyAsync(&acc, ctx->d_sound, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out->rays_reaching_listener = acc.reaching;
    out->direct_hits = acc.direct_hits;
    out->direct_energy_sum = acc.direct_energy_sum;
    out->traces = acc.traces;
    out->occlusion_attenuation = acc.occlusion;
    // TotalEnergy /= RaycastsPerTick (FSAC.cpp:294); every reaching ray returns Energy == 1
    out->total_energy = p->raycasts_per_tick > 0 ? (float)acc.reaching / (float)p->raycasts_per_tick : 0.0f;
    s->occlusion = acc.occlusion;
    return FS_OK;
}

int fs_get_occlusion_attenuation(fs_context* ctx, fs_source h, float* out) {
    if (!ctx || !out) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return FS_ERR_BAD_HANDLE;
    *out = s->occlusion;
    return FS_OK;
}

// ---- engine line trace ------------------------------------------------------------------------------------
int fs_trace_rays(fs_context* ctx, const float* origins, const float* dirs, const float* tmax, int32_t N,
                  int32_t any_hit, int32_t* hit, float* t, int32_t* tri, float* normal) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    { int ir = maybe_install_refined(ctx); if (ir) return ir; }                     // fs_scene_commit_progressive: the better tree is ready
    if (ctx->refit_pending) { int rr = fs_scene_refit(ctx); if (rr) return rr; }   // moved triangles: refit before tracing
    if (N < 0 || (N > 0 && (!origins || !dirs || !tmax || !hit))) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad ray arrays");
    if (any_hit != 1 && N > 0 && (!t || !tri || !normal)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "closest-hit outputs required");
    if (any_hit < 0 || any_hit > 8) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "any_hit: 0 closest, 1 any, 2 .. 8 closest by the cooperative traversal");
    if (N == 0) return FS_OK;
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    float *d_o = nullptr, *d_d = nullptr, *d_tm = nullptr, *d_t = nullptr, *d_n = nullptr;
    int32_t *d_hit = nullptr, *d_tri = nullptr;
    size_t n3 = sizeof(float) * 3 * (size_t)N, n1 = sizeof(float) * (size_t)N;
    int rc = FS_OK;
    auto cleanup = [&]() {
        (void)hipFree(d_o); (void)hipFree(d_d); (void)hipFree(d_tm); (void)hipFree(d_t); (void)hipFree(d_n);
        (void)hipFree(d_hit); (void)hipFree(d_tri);
    };
#define FS_TRY(call)                                                   \
    do {                                                               \
        hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) { rc = ctx->hip_fail(e_, #call); cleanup(); return rc; } \
    } while (0)
    FS_TRY(hipMalloc((void**)&d_o, n3));
    FS_TRY(hipMalloc((void**)&d_d, n3));
    FS_TRY(hipMalloc((void**)&d_tm, n1));
    FS_TRY(hipMalloc((void**)&d_t, n1));
    FS_TRY(hipMalloc((void**)&d_n, n3));
    FS_TRY(hipMalloc((void**)&d_hit, n1 + sizeof(int32_t)));   // (+ the cooperative traversal's overflow word)
    FS_TRY(hipMemsetAsync(d_hit + N, 0, sizeof(int32_t), ctx->stream));
    FS_TRY(hipMalloc((void**)&d_tri, n1));
    FS_TRY(hipMemcpyAsync(d_o, origins, n3, hipMemcpyHostToDevice, ctx->stream));
    FS_TRY(hipMemcpyAsync(d_d, dirs, n3, hipMemcpyHostToDevice, ctx->stream));
    FS_TRY(hipMemcpyAsync(d_tm, tmax, n1, hipMemcpyHostToDevice, ctx->stream));
    launch_trace_rays(ctx->scene, d_o, d_d, d_tm, N, any_hit, d_hit, d_t, d_tri, d_n, ctx->stream);
    FS_TRY(hipGetLastError());
    FS_TRY(hipMemcpyAsync(hit, d_hit, n1, hipMemcpyDeviceToHost, ctx->stream));
    int32_t coop_overflow = 0;
    FS_TRY(hipMemcpyAsync(&coop_overflow, d_hit + N, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (any_hit != 1) {
        FS_TRY(hipMemcpyAsync(t, d_t, n1, hipMemcpyDeviceToHost, ctx->stream));
        FS_TRY(hipMemcpyAsync(tri, d_tri, n1, hipMemcpyDeviceToHost, ctx->stream));
        FS_TRY(hipMemcpyAsync(normal, d_n, n3, hipMemcpyDeviceToHost, ctx->stream));
    }
    FS_TRY(hipStreamSynchronize(ctx->stream));
#undef FS_TRY
    cleanup();
    if (coop_overflow) return ctx->fail(FS_ERR_OVERFLOW, "cooperative traversal: a group's node stack overflowed");
    return FS_OK;
}

// ---- f1: text import / export (FSAC.cpp:454-505) ------------------------------------------------------------
extern "C++" {
namespace {
// FString::SanitizeFloat(double, MinFractionalDigits = 1): "%f", trailing zeros trimmed, one fractional digit kept
std::string sanitize_float(double v) {
    if (v == 0.0) v = 0.0;  // strip negative zero
    char buf[512];
    std::snprintf(buf, sizeof(buf), "%f", v);
    std::string t(buf);
    bool numeric = !t.empty();
    for (size_t i = 0; i < t.size(); ++i) {
        char c = t[i];
        if (!((c >= '0' && c <= '9') || c == '.' || ((c == '-' || c == '+') && i == 0))) numeric = false;
    }
    if (!numeric) return t;  // "nan", "inf": left alone like the engine
    size_t dot = t.find('.');
    if (dot == std::string::npos) return t + ".0";
    size_t end = t.size();
    while (end > dot + 2 && t[end - 1] == '0') --end;
    return t.substr(0, end);
}
}  // namespace
}  // extern "C++"

int fs_save_array_to_file(const float* data, int32_t n, const char* path) {
    if (!path || n < 0 || (n > 0 && !data)) return FS_ERR_INVALID_ARGUMENT;
    FILE* f = std::fopen(path, "wb");
    if (!f) return FS_ERR_INVALID_ARGUMENT;
    for (int32_t i = 0; i < n; ++i) {   // FString::Join(Lines, "\n"): no trailing newline
        std::string s = sanitize_float((double)data[i]);
        if (i) std::fputc('\n', f);
        std::fwrite(s.data(), 1, s.size(), f);
    }
    std::fclose(f);
    return FS_OK;
}

int fs_load_float_array(const char* path, float* out, int32_t cap, int32_t* n_out) {
    if (!path || !n_out || cap < 0) return FS_ERR_INVALID_ARGUMENT;
    *n_out = 0;
    FILE* f = std::fopen(path, "rb");
    if (!f) return FS_ERR_INVALID_ARGUMENT;   // "Failed to load impulse response file" FSAC.cpp:472
    std::string content;
    char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) content.append(buf, got);
    std::fclose(f);
    int32_t n = 0;
    size_t pos = 0;
    while (pos <= content.size()) {
        size_t nl = content.find('\n', pos);
        if (nl == std::string::npos) nl = content.size();
        if (nl > pos) {                   // ParseIntoArray(..., InCullEmpty = true)
            std::string line = content.substr(pos, nl - pos);
            float v = (float)std::atof(line.c_str());   // FCString::Atof
            if (out && n < cap) out[n] = v;
            ++n;
        }
        pos = nl + 1;
    }
    *n_out = n;
    return FS_OK;
}

int fs_save_impulse_response(fs_context* ctx, fs_source h, int32_t channel, const char* path) {
    if (!ctx || !path) return FS_ERR_INVALID_ARGUMENT;
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    const float* p = nullptr;
    int32_t n = 0;
    int rc = fs_get_impulse_response(ctx, h, channel, &p, &n);
    if (rc) return rc;
    return fs_save_array_to_file(p, n, path);
}

// ---- f2: reverb convolution (RVB.cpp:74-213) ---------------------------------------------------------------------
static int alloc_fade(fs_context* ctx, Source* s);

int fs_reverb_init(fs_context* ctx, fs_source h, int32_t frame_size) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (frame_size < 1 || frame_size > 16384 || ctx->num_samples - 1 > kReverbRing)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad reverb frame size / IR longer than the history ring");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    // Reconstructs on the compute stream record an event for the callbacks only for a source that has a reverb: the ones
    // already in flight finish before this source gets one.
    FS_FLUSH(ctx);
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->rev_stream));
    if (s->d_ring) { (void)hipFree(s->d_ring); (void)hipFree(s->d_rev_in); (void)hipFree(s->d_rev_cur); (void)hipFree(s->d_rev_out); }
    if (s->d_fade_from) { (void)hipFree(s->d_fade_from); (void)hipFree(s->d_fade_to); }
    s->d_ring = s->d_rev_in = s->d_rev_cur = s->d_rev_out = s->d_fade_from = s->d_fade_to = nullptr;
    FS_HIP(ctx, hipMalloc((void**)&s->d_ring, sizeof(float) * 2 * kReverbRing));
    FS_HIP(ctx, hipMalloc((void**)&s->d_rev_in, sizeof(float) * 2 * (size_t)frame_size));
    FS_HIP(ctx, hipMalloc((void**)&s->d_rev_cur, sizeof(float) * 2 * (size_t)frame_size));
    FS_HIP(ctx, hipMalloc((void**)&s->d_rev_out, sizeof(float) * 2 * (size_t)frame_size));
    FS_HIP(ctx, hipMemsetAsync(s->d_ring, 0, sizeof(float) * 2 * kReverbRing, ctx->rev_stream));   // SetNumZeroed
    s->rev_head = 0;
    s->rev_frame = frame_size;
    s->fading = s->fade_primed = false;   // (the first callback takes the IR unfaded)
    if (s->fade_len > 0) return alloc_fade(ctx, s);
    return FS_OK;
}

// fs_reverb_set_crossfade: the callback's two IR copies, once the source has a reverb and a fade length
static int alloc_fade(fs_context* ctx, Source* s) {
    const size_t bytes = sizeof(float) * (size_t)ctx->num_samples;
    if (!s->d_fade_from) FS_HIP(ctx, hipMalloc((void**)&s->d_fade_from, bytes));
    if (!s->d_fade_to) FS_HIP(ctx, hipMalloc((void**)&s->d_fade_to, bytes));
    return FS_OK;
}

int fs_reverb_set_crossfade(fs_context* ctx, fs_source h, int32_t samples) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (samples < 0 || (int64_t)samples > 4 * (int64_t)ctx->cfg.sample_rate)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "crossfade length out of range (0 = off, 1 .. 4 * sample_rate)");
    if (samples > 0 && s->d_ring) {
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        const int rc = alloc_fade(ctx, s);
        if (rc) return rc;
    }
    if (s->fade_len == 0) s->fade_primed = false;   // enabling: nothing to fade from
    s->fading = false;                              // a running fade ends at its target IR
    s->fade_len = samples;
    return FS_OK;
}

int fs_reverb_process(fs_context* ctx, fs_source h, const float* in, float* out, int32_t apply_reverb, uint32_t flags) {
    if (!ctx || !in || !out) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (!s->d_ring) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init has not been called for this source");
    const int frame = s->rev_frame;
    if (!apply_reverb) {   // bApplyReverb == false: RVB.cpp:128-132
        std::memcpy(out, in, sizeof(float) * 2 * (size_t)frame);
        return FS_OK;
    }
    if (s->fade_len > 0 && (!s->d_fade_from || !s->d_fade_to))   // (fs_reverb_init could not allocate them)
        return ctx->fail(FS_ERR_OUT_OF_MEMORY, "the crossfade's impulse-response buffers are missing: call fs_reverb_init again");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    // Audio thread.  The callback has its own stream: it is never queued behind a traced frame on the compute stream.
    // The device-resident IR is written by reconstructs on the tail stream: read it behind the newest one and make the
    // next one wait for this read — both through events, exchanged with the game thread under the source's ir_mu.
    // With a crossfade (fs_reverb_set_crossfade) the callback convolves its own copies of the IR: it reads d_ir_mono only when a
    // newer IR is there (ir_gen), once, into h_to — only then does it wait for the write and make the next one wait for it.
    hipStream_t rs = ctx->rev_stream;
    const bool xfade = s->fade_len > 0;
    const int literal = (flags & FS_REVERB_LITERAL_TAIL) ? 1 : 0;
    {
        std::lock_guard<std::mutex> g(s->ir_mu);
        const bool take = xfade && (!s->fade_primed || s->ir_gen != s->fade_gen);
        if ((!xfade || take) && s->last_rec >= 0) FS_HIP(ctx, stream_waits_for_rec(ctx, rs, s, s->last_rec));
        if (take) {
            float a = 0.0f;
            if (s->fade_primed) {   // a fade from what is heard now: h_to alone, or the mix at the last output sample of a running fade
                if (s->fading) a = (float)s->fade_pos / (float)s->fade_len;
                else std::swap(s->d_fade_from, s->d_fade_to);
                s->fading = true;
                s->fade_pos = 0;
            }
            launch_reverb_fade_start(s->d_fade_from, s->d_fade_to, s->d_ir_mono, ctx->num_samples, a, rs);
            FS_HIP(ctx, hipGetLastError());
            FS_HIP(ctx, hipEventRecord(s->ev_rev, rs));
            s->rev_recorded = true;
            s->fade_primed = true;
            s->fade_gen = s->ir_gen;
        }
        FS_HIP(ctx, hipMemcpyAsync(s->d_rev_in, in, sizeof(float) * 2 * (size_t)frame, hipMemcpyHostToDevice, rs));
        if (!xfade)
            launch_reverb(s->d_ir_mono, ctx->num_samples, s->d_ring, s->rev_head, s->d_rev_in, s->d_rev_cur, s->d_rev_out, frame, literal, rs);
        else if (s->fading)
            launch_reverb(s->d_fade_from, ctx->num_samples, s->d_ring, s->rev_head, s->d_rev_in, s->d_rev_cur, s->d_rev_out, frame, literal, rs,
                          s->d_fade_to, s->fade_pos, s->fade_len);
        else
            launch_reverb(s->d_fade_to, ctx->num_samples, s->d_ring, s->rev_head, s->d_rev_in, s->d_rev_cur, s->d_rev_out, frame, literal, rs);
        FS_HIP(ctx, hipGetLastError());
        if (!xfade) {
            FS_HIP(ctx, hipEventRecord(s->ev_rev, rs));
            s->rev_recorded = true;
        }
    }
    s->rev_head += (unsigned)frame;
    if (s->fading && (s->fade_pos += frame) >= s->fade_len) s->fading = false;   // complete: h_from := h_to, one convolution again
    FS_HIP(ctx, hipMemcpyAsync(out, s->d_rev_out, sizeof(float) * 2 * (size_t)frame, hipMemcpyDeviceToHost, rs));
    FS_HIP(ctx, hipStreamSynchronize(rs));
    return FS_OK;
}

// fs_reverb_process_batch: the staging of one call (fs_context::h_rev_stage / d_rev_stage), every block 256-byte aligned
extern "C++" {
namespace {
struct RevStageLayout {
    size_t items, lists, in, up_bytes;      // host and device, the same offsets: what goes up in one copy
    size_t h_out, h_mix, host_bytes;        // host: what comes back
    size_t d_cur, d_out, d_mix, dev_bytes;  // device: out | mix adjacent, one copy back
};
size_t rev_align(size_t b) { return (b + 255) & ~(size_t)255; }
RevStageLayout rev_stage_layout(int count, int frame) {
    const size_t rows = sizeof(float) * 2 * (size_t)frame * (size_t)count, row = sizeof(float) * 2 * (size_t)frame;
    RevStageLayout l;
    l.items = 0;
    l.lists = rev_align(sizeof(ReverbItem) * (size_t)count);
    l.in = l.lists + rev_align(sizeof(int) * 3 * (size_t)count);
    l.up_bytes = l.in + rows;
    l.h_out = rev_align(l.up_bytes);
    l.h_mix = l.h_out + rows;   // (adjacent to out: rows is a multiple of 8 bytes)
    l.host_bytes = l.h_mix + row;
    l.d_cur = rev_align(l.up_bytes);
    l.d_out = l.d_cur + rev_align(rows);
    l.d_mix = l.d_out + rows;
    l.dev_bytes = l.d_mix + row;
    return l;
}
}  // namespace
}  // extern "C++"

int fs_reverb_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in, float* out,
                            const int32_t* apply_reverb, uint32_t flags, float* mix) {
    if (!ctx || !sources || !in || (!out && !mix)) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    if (count < 1 || count > FS_MAX_REVERB_BATCH)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "count out of range (1 .. FS_MAX_REVERB_BATCH)");
    // Everything is validated before the first state change or enqueue: a refused call changes nothing.
    std::vector<Source*> srcs((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        Source* s = srcs[(size_t)i] = get_source(ctx, sources[i]);
        if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
        if (!s->d_ring) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_reverb_init has not been called for this source");
        if (s->rev_frame != srcs[0]->rev_frame) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "the sources of a batch share one frame size");
        if ((!apply_reverb || apply_reverb[i]) && s->fade_len > 0 && (!s->d_fade_from || !s->d_fade_to))
            return ctx->fail(FS_ERR_OUT_OF_MEMORY, "the crossfade's impulse-response buffers are missing: call fs_reverb_init again");
    }
    std::vector<int32_t> order((size_t)count);   // rows by ascending Source*: the one locking order of every thread (fs_capi_publish.cpp)
    for (int32_t i = 0; i < count; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return srcs[(size_t)a] < srcs[(size_t)b]; });
    for (int32_t k = 1; k < count; ++k)
        if (srcs[(size_t)order[(size_t)k]] == srcs[(size_t)order[(size_t)k - 1]])
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "a source appears twice in the batch");
    const int frame = srcs[0]->rev_frame;
    const size_t row = 2 * (size_t)frame;   // floats
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t rs = ctx->rev_stream;
    const RevStageLayout l = rev_stage_layout(count, frame);
    if (l.host_bytes > ctx->rev_stage_host || l.dev_bytes > ctx->rev_stage_dev) {   // first call of this size (every call ends synchronised: nothing reads the old one)
        if (ctx->h_rev_stage) (void)hipHostFree(ctx->h_rev_stage);
        if (ctx->d_rev_stage) (void)hipFree(ctx->d_rev_stage);
        ctx->h_rev_stage = ctx->d_rev_stage = nullptr; ctx->rev_stage_host = ctx->rev_stage_dev = 0;
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_rev_stage, l.host_bytes, hipHostMallocDefault));
        ctx->rev_stage_host = l.host_bytes;
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_rev_stage, l.dev_bytes));
        ctx->rev_stage_dev = l.dev_bytes;
    }
    char* hs = ctx->h_rev_stage; char* ds = ctx->d_rev_stage;
    ReverbItem* items = (ReverbItem*)(hs + l.items);
    int* plain = (int*)(hs + l.lists); int* fade = plain + count; int* take = fade + count;
    int n_plain = 0, n_fade = 0, n_take = 0;
    float* h_in = (float*)(hs + l.in);
    for (int32_t i = 0; i < count; ++i)   // (a bypassed row goes up only for the mix)
        if (mix || !apply_reverb || apply_reverb[i])
            std::memcpy(h_in + (size_t)i * row, in + (size_t)i * row, sizeof(float) * row);
    const int literal = (flags & FS_REVERB_LITERAL_TAIL) ? 1 : 0;
    {
        // Per source what fs_reverb_process does under ir_mu, in list order; the locks of all convolved sources are held while the
        // work is enqueued (a reconstruct that found one free would not wait for a read this call has yet to record), not longer.
        std::vector<std::unique_lock<std::mutex>> locks;
        locks.reserve((size_t)count);
        for (int32_t i : order)
            if (!apply_reverb || apply_reverb[i]) locks.emplace_back(srcs[(size_t)i]->ir_mu);
        for (int32_t i = 0; i < count; ++i) {
            Source* s = srcs[(size_t)i];
            ReverbItem& it = items[i];
            std::memset(&it, 0, sizeof(it));
            if (apply_reverb && !apply_reverb[i]) continue;   // the bypass touches no state
            it.apply = 1;
            const bool xfade = s->fade_len > 0;
            const bool tk = xfade && (!s->fade_primed || s->ir_gen != s->fade_gen);
            if ((!xfade || tk) && s->last_rec >= 0) {
                const int buf = s->last_rec;
                // (a finished reconstruct needs no barrier packet on the stream: S of them are most of a short batch)
                bool done = false;
                if (s->rec_recorded[buf] && !s->rec_batch[buf]) {
                    done = hipEventQuery(s->ev_rec[buf]) == hipSuccess;
                    if (!done) (void)hipGetLastError();   // hipErrorNotReady is not an error
                }
                if (!done) FS_HIP(ctx, stream_waits_for_rec(ctx, rs, s, buf));
            }
            if (tk) {
                float a = 0.0f;
                if (s->fade_primed) {   // a fade from what is heard now: h_to alone, or the mix at the last output sample of a running fade
                    if (s->fading) a = (float)s->fade_pos / (float)s->fade_len;
                    else std::swap(s->d_fade_from, s->d_fade_to);
                    s->fading = true;
                    s->fade_pos = 0;
                }
                it.take_from = s->d_fade_from; it.take_to = s->d_fade_to; it.take_ir = s->d_ir_mono; it.take_a = a;
                take[n_take++] = i;
                s->rev_recorded = true;   // (ev_rev is recorded behind the fade-start launch below, still under the lock)
                s->fade_primed = true;
                s->fade_gen = s->ir_gen;
            }
            it.ring = s->d_ring;
            it.head = s->rev_head;
            if (!xfade) { it.ir = s->d_ir_mono; plain[n_plain++] = i; s->rev_recorded = true; }
            else if (s->fading) {
                it.ir = s->d_fade_from; it.ir_to = s->d_fade_to; it.fade_pos = s->fade_pos; it.fade_len = s->fade_len;
                fade[n_fade++] = i;
            } else { it.ir = s->d_fade_to; plain[n_plain++] = i; }
            s->rev_head += (unsigned)frame;
            if (s->fading && (s->fade_pos += frame) >= s->fade_len) s->fading = false;   // complete: h_from := h_to, one convolution again
        }
        FS_HIP(ctx, hipMemcpyAsync(ds, hs, l.up_bytes, hipMemcpyHostToDevice, rs));
        const ReverbItem* d_items = (const ReverbItem*)(ds + l.items);
        const int* d_plain = (const int*)(ds + l.lists);
        if (n_take) {
            launch_reverb_batch_fade_start(d_items, d_plain + 2 * count, n_take, ctx->num_samples, rs);
            FS_HIP(ctx, hipGetLastError());
            for (int k = 0; k < n_take; ++k) FS_HIP(ctx, hipEventRecord(srcs[(size_t)take[k]]->ev_rev, rs));
        }
        ReverbBatch b{};
        b.items = d_items;
        b.plain = d_plain; b.n_plain = n_plain;
        b.fade = d_plain + count; b.n_fade = n_fade;
        b.count = count; b.frame = frame; b.ir_size = ctx->num_samples; b.literal_tail = literal;
        b.in = (const float*)(ds + l.in);
        b.cur = (float*)(ds + l.d_cur);
        b.out = (float*)(ds + l.d_out);
        b.mix = mix ? (float*)(ds + l.d_mix) : nullptr;
        launch_reverb_batch(b, rs);
        FS_HIP(ctx, hipGetLastError());
        for (int k = 0; k < n_plain; ++k) {   // without a crossfade the convolution itself reads d_ir_mono
            Source* s = srcs[(size_t)plain[k]];
            if (s->fade_len == 0) FS_HIP(ctx, hipEventRecord(s->ev_rev, rs));
        }
    }
    if (out)   // out | mix are adjacent on both sides: one copy back
        FS_HIP(ctx, hipMemcpyAsync(hs + l.h_out, ds + l.d_out, sizeof(float) * row * ((size_t)count + (mix ? 1 : 0)), hipMemcpyDeviceToHost, rs));
    else
        FS_HIP(ctx, hipMemcpyAsync(hs + l.h_mix, ds + l.d_mix, sizeof(float) * row, hipMemcpyDeviceToHost, rs));
    FS_HIP(ctx, hipStreamSynchronize(rs));
    if (out) {
        const float* h_out = (const float*)(hs + l.h_out);
        for (int32_t i = 0; i < count; ++i) {   // bApplyReverb == false: RVB.cpp:128-132
            const float* from = (apply_reverb && !apply_reverb[i]) ? in + (size_t)i * row : h_out + (size_t)i * row;
            if (from != out + (size_t)i * row) std::memcpy(out + (size_t)i * row, from, sizeof(float) * row);   // (in place: in == out)
        }
    }
    if (mix) std::memcpy(mix, hs + l.h_mix, sizeof(float) * row);
    return FS_OK;
}

int fs_reverb_release(fs_context* ctx, fs_source h) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    Source* s = get_source(ctx, h);
    if (!s) return ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    if (s->d_ring && ctx->device_ok) {
        FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
        FS_HIP(ctx, hipMemsetAsync(s->d_ring, 0, sizeof(float) * 2 * kReverbRing, ctx->rev_stream));
        s->rev_head = 0;
        s->fading = false;   // a running crossfade ends at its target IR
    }
    return FS_OK;
}

// ---- row f4: UMaterialAcousticProcessor::ApplyMaterialFD (MaterialAcousticProcessor.cpp:8-107) -----------------
int fs_apply_material_fd(fs_context* ctx, const float* in, int32_t L, const float* absorption, const float* transmission,
                         const float* scattering, int32_t num_responses, float* specular, float* diffuse,
                         float* transmitted) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (L < 0 || L > (1 << 24)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "block length out of range (0 .. 2^24)");
    if (!absorption || !transmission || !scattering) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "null response curve");
    if (L > 0 && (!in || !specular || !diffuse || !transmitted)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "null buffer");
    int n = 0;
    while ((1 << n) < L) ++n;                                      // MAP.cpp:15-16: next power of two
    const int N = 1 << n, bins = N / 2 + 1;
    if (num_responses != bins)                                     // MAP.cpp:20-26
        return ctx->fail(FS_ERR_SIZE_MISMATCH, "all response curves must have length " + std::to_string(bins));
    if (L == 0) return FS_OK;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no device");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (n > ctx->fft_cap_n || L > ctx->fft_cap_l) {
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (void* p : {(void*)ctx->d_fft_x, (void*)ctx->d_fft_y, (void*)ctx->d_fft_w, (void*)ctx->d_fft_in,
                        (void*)ctx->d_fft_resp, (void*)ctx->d_fft_out})
            if (p) (void)hipFree(p);
        ctx->d_fft_x = ctx->d_fft_y = ctx->d_fft_w = nullptr;
        ctx->d_fft_in = ctx->d_fft_resp = ctx->d_fft_out = nullptr;
        ctx->fft_cap_n = -1; ctx->fft_cap_l = 0; ctx->fft_n = -1;
        if (ctx->fft_graph) { (void)hipGraphExecDestroy(ctx->fft_graph); ctx->fft_graph = nullptr; }   // captured the old buffers
        ctx->fft_graph_n = -1;
        const int cn = std::max(n, ctx->fft_cap_n);
        const size_t CN = (size_t)1 << cn;
        FS_HIP(ctx, hipMalloc(&ctx->d_fft_x, sizeof(float2) * CN));
        FS_HIP(ctx, hipMalloc(&ctx->d_fft_y, sizeof(float2) * 3 * CN));
        FS_HIP(ctx, hipMalloc(&ctx->d_fft_w, sizeof(float2) * std::max<size_t>(CN / 2, 1)));
        FS_HIP(ctx, hipMalloc(&ctx->d_fft_in, sizeof(float) * CN));
        FS_HIP(ctx, hipMalloc(&ctx->d_fft_resp, sizeof(float) * 3 * (CN / 2 + 1)));
        FS_HIP(ctx, hipMalloc(&ctx->d_fft_out, sizeof(float) * 3 * CN));
        ctx->fft_cap_n = cn; ctx->fft_cap_l = (int)CN;
    }
    if (ctx->fft_n != n) {   // twiddles in double precision: W[k] = exp(-2 pi i k / N)
        std::vector<float2> w(std::max(N / 2, 1));
        for (int k = 0; k < N / 2; ++k) {
            const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)N;
            w[(size_t)k] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        if (N < 2) w[0] = make_float2(1.f, 0.f);
        FS_HIP(ctx, hipMemcpyAsync(ctx->d_fft_w, w.data(), sizeof(float2) * w.size(), hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));   // w is a stack-owned staging buffer
        ctx->fft_n = n;
    }
    if (L > (1 << 17)) {   // large blocks are copy-bound, not launch-bound: straight from / to the caller's memory
        FS_HIP(ctx, hipMemcpyAsync(ctx->d_fft_in, in, sizeof(float) * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(ctx, hipMemcpyAsync(ctx->d_fft_resp, absorption, sizeof(float) * bins, hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(ctx, hipMemcpyAsync(ctx->d_fft_resp + bins, transmission, sizeof(float) * bins, hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(ctx, hipMemcpyAsync(ctx->d_fft_resp + 2 * bins, scattering, sizeof(float) * bins, hipMemcpyHostToDevice, ctx->stream));
        launch_apply_material_fd(ctx->d_fft_in, L, n, ctx->d_fft_x, ctx->d_fft_y, ctx->d_fft_w, ctx->d_fft_resp, ctx->d_fft_out,
                                 ctx->stream);
        FS_HIP(ctx, hipGetLastError());
        FS_HIP(ctx, hipMemcpyAsync(specular, ctx->d_fft_out, sizeof(float) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(ctx, hipMemcpyAsync(diffuse, ctx->d_fft_out + L, sizeof(float) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(ctx, hipMemcpyAsync(transmitted, ctx->d_fft_out + 2 * (size_t)L, sizeof(float) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FS_OK;
    }
    // pinned staging so that the captured copies always use the same addresses
    const size_t stage_floats = (size_t)L + 3 * (size_t)bins + 3 * (size_t)L;
    if (stage_floats > ctx->fft_stage_floats) {
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->fft_graph) { (void)hipGraphExecDestroy(ctx->fft_graph); ctx->fft_graph = nullptr; ctx->fft_graph_n = -1; }
        if (ctx->h_fft_stage) (void)hipHostFree(ctx->h_fft_stage);
        ctx->h_fft_stage = nullptr; ctx->fft_stage_floats = 0;
        FS_HIP(ctx, hipHostMalloc((void**)&ctx->h_fft_stage, sizeof(float) * stage_floats, hipHostMallocDefault));
        ctx->fft_stage_floats = stage_floats;
    }
    float* h_in = ctx->h_fft_stage;
    float* h_resp = h_in + L;
    float* h_out = h_resp + 3 * (size_t)bins;
    std::memcpy(h_in, in, sizeof(float) * (size_t)L);
    std::memcpy(h_resp, absorption, sizeof(float) * (size_t)bins);
    std::memcpy(h_resp + bins, transmission, sizeof(float) * (size_t)bins);
    std::memcpy(h_resp + 2 * (size_t)bins, scattering, sizeof(float) * (size_t)bins);
    auto enqueue = [&](hipStream_t st) -> hipError_t {
        hipError_t e = hipMemcpyAsync(ctx->d_fft_in, h_in, sizeof(float) * (size_t)L, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(ctx->d_fft_resp, h_resp, sizeof(float) * 3 * (size_t)bins, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        launch_apply_material_fd(ctx->d_fft_in, L, n, ctx->d_fft_x, ctx->d_fft_y, ctx->d_fft_w, ctx->d_fft_resp,
                                 ctx->d_fft_out, st);
        return hipMemcpyAsync(h_out, ctx->d_fft_out, sizeof(float) * 3 * (size_t)L, hipMemcpyDeviceToHost, st);
    };
    if (ctx->fft_graph_n != n || ctx->fft_graph_l != L) {   // (re)capture for this block size
        if (ctx->fft_graph) { (void)hipGraphExecDestroy(ctx->fft_graph); ctx->fft_graph = nullptr; }
        ctx->fft_graph_n = -1;
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            hipError_t e = enqueue(ctx->stream);
            hipError_t e2 = hipStreamEndCapture(ctx->stream, &g);
            if (e == hipSuccess && e2 == hipSuccess && g &&
                hipGraphInstantiate(&ctx->fft_graph, g, nullptr, nullptr, 0) == hipSuccess) {
                ctx->fft_graph_n = n; ctx->fft_graph_l = L;
            } else {
                ctx->fft_graph = nullptr;
            }
            if (g) (void)hipGraphDestroy(g);
        }
        (void)hipGetLastError();
    }
    if (ctx->fft_graph) FS_HIP(ctx, hipGraphLaunch(ctx->fft_graph, ctx->stream));
    else FS_HIP(ctx, enqueue(ctx->stream));   // capture unavailable: the same sequence, launched one by one
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(specular, h_out, sizeof(float) * (size_t)L);
    std::memcpy(diffuse, h_out + L, sizeof(float) * (size_t)L);
    std::memcpy(transmitted, h_out + 2 * (size_t)L, sizeof(float) * (size_t)L);
    return FS_OK;
}

}  // extern "C"
