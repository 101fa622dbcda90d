// fs_context.hpp — the context behind the C ABI (include/frequensee.h) and the helpers its translation units share.
// Internal: included by fs_capi_context.cpp (lifetime, helpers, stats), fs_capi_scene.cpp (geometry, commits, refit),
// fs_capi_frame.cpp (sources, the traced frame: describe / resources / commit / launch), fs_capi_pipeline.cpp (held frames, the
// drain), fs_capi_publish.cpp (reconstruct + publish: the IR ring, the host word, the fused launch's reconstruct parts),
// fs_capi_ir.cpp (reconstruct / tick / IR / energy entry points), fs_capi_comm.cpp (RCCL behind the ABI), fs_capi_reverb.cpp
// (the reverb callback, and the staging, layout and tail of all three audio callbacks), fs_capi_paths.cpp (the five path queries),
// fs_capi_direct_render.cpp (the direct-sound callback, and what the two renderers share on the host), fs_capi_reflect_render.cpp
// (the early-reflection callback) and fs_capi_aux.cpp (legacy tracer, line trace, text interchange, material FD).
//
// Mirrors the roles of UAudioRayTracingSubsystem (context lifetime, geometry/source registries,
// per-source update: AudioRayTracingSubsystem.cpp:32-53, 128-195) and of UFrequenSeeAudioComponent's
// buffers (EnergyBuffer, ImpulseBuffer: FrequenSeeAudioComponent.h:69-91, 113, 133-143).  All compute
// is HIP on the context's streams; there is no CPU fallback.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is opened at run time (fs_comm_*), never linked

#include "fs_internal.hpp"

using namespace fs;

namespace fsi {

constexpr int kIrRing = 8;  // published IR ring: up to 7 publishes of a source in flight (grouped frames of one source finish
                            // together); a returned pointer stays valid until the 7th-next publish (3 and "second-next" until round 3)

// Energy buffers per source, used in rotation: frame f deposits into one while the tail stream still reduces /
// reconstructs frame f - 1 from another; pipelined frames finish frame f - 2 only in the launch that plans frame f
// (and flushes ITS buffer), so that a fourth one lets frame f + 1 start without waiting for that tail.
// Frames in flight.  A pipelined frame lives through several launches — plan, its walk (one launch, or one launch per
// stage of a staged depth = 0 walk), connect — while the frames behind it are in their earlier steps; everything a
// frame owns rotates with the frame index.  kMaxSets bounds the rotation: energy buffers per source (zeroed by the
// plan pass of frame f, deposited into up to kMaxWalkParts + 1 launches later, then read by the tail), frame scratch
// sets (plan counts, cursors, work counters), per-frame tables of batched frames.  The big per-frame arrays (subpath
// state, segment records, schedules, continuation records) come in fs_context::state_sets sets, as many as the deepest
// pipeline in use needs (3 until a staged walk is pipelined).
constexpr int kMaxSets = 12;
// Energy buffers of a source.  A frame OWNS its buffer from the launch that plans it (and zeroes the buffer) to the launch
// that reconstructs it: stages + 3 launches for a staged depth = 0 frame, times the frames of the source per launch
// (fs_set_frames_per_launch).  Up to two frames per launch rotate through the first kEnergyBufsBase (11 launches x 2 at
// most; with 2 or 3 frames per launch the rotation then repeats every kBatchSlots launches or sooner, which is what lets a
// batched frame find its table already on the device — 48 buffers at two per launch: 928 -> 914 M rays/s); three and four
// per launch rotate through all kEnergyBufs (11 launches x 4), the buffers beyond the base allocated at their first use.
// frame_resources never hands out a buffer that a frame in flight still owns, whatever the rotation says (round 3 did:
// four staged frames per launch wrapped the 24-buffer rotation after six launches and zeroed buffers still being deposited into).
constexpr int kEnergyBufsBase = 2 * kMaxSets;
constexpr int kEnergyBufs = 4 * kMaxSets;
constexpr int kScratchSets = kMaxSets;
static_assert(kMaxSets >= kMaxWalkParts + 3, "a staged frame is in flight for stages + 2 launches and its buffer is read one more");
static_assert(kEnergyBufs >= 4 * (kMaxWalkParts + 3), "four frames of one source per launch, each owning its buffer for stages + 3 launches");

// Events that order work of two streams of the SAME device (the compute stream's hand-over to the tail stream, the sum over the
// ranks back to the compute stream, the reverb stream's reads): a DEVICE-scope release.  The default — a system-scope fence when
// the event is recorded — writes every dirty L2 line back and invalidates the caches: behind a frame kernel that has just written
// 100 MB of records that is tens of microseconds in which nothing runs, and the next launch starts on cold caches
// (tools/rccl_tax.sh: a one-rank communicator cost 7.5 % of the plain rate with default events).  Events the HOST inspects
// before it reads host memory (the publishes' ev[slot], tail_batch_ev) keep the system scope.
constexpr unsigned kDeviceEventFlags = hipEventDisableTiming | hipEventReleaseToDevice;

// What fs_direct_render_init / fs_reflection_render_init gave a source (the audio thread's, like the reverb fields): the state
// block on the device — the renderer's header, then the history rings [2][ring] — and what the source was initialised with;
// table is one of fs_context::dr_tables' (owned by the context); max_delay = D, the largest delay in samples
struct RenderSetup {
    char* d = nullptr;
    int frame = 0, taps = 0, max_delay = 0;
    unsigned ring = 0;
    const float* table = nullptr;
};
// A renderer's voice bank on a source (fs_reflection_render_init / fs_binaural_render_init / fs_ambisonic_render_init): the
// set-up — its header is a VoiceBankState, kVoiceBankHeader bytes (the ambisonic renderer's: kAmbisonicBankHeader); the rings
// (two; the ambisonic renderer's: one) are shared by the `voices` slots — and the slot table the callback matches against, the
// host's copy (the device's is in the state block)
struct VoiceBank {
    RenderSetup r;
    int voices = 0;
    int order = 0;   // (the ambisonic renderer's: what fs_ambisonic_render_init was given)
    bool held[FS_MAX_REFLECTION_VOICES] = {};
    uint32_t key[FS_MAX_REFLECTION_VOICES] = {};
    void free_slots() {
        for (int j = 0; j < FS_MAX_REFLECTION_VOICES; ++j) { held[j] = false; key[j] = 0; }
    }
};

struct Source {
    bool alive = false;
    float pos[3] = {0, 0, 0};
    uint32_t object = FS_NO_OBJECT;    // the actor this source belongs to: its own walks ignore it (fs_source_set_object)
    // directivity (fs_source_set_orientation / fs_source_set_directivity): unit forward vector and the device table [B][dir_samples]
    // (null: omnidirectional).  A new table is a new allocation: the one it replaces may still be read by an enqueued frame
    // (fs_context::retired_tables)
    float fwd[3] = {1.0f, 0.0f, 0.0f};
    float* d_dir = nullptr;
    int32_t dir_samples = 0;
    // order window (fs_source_set_order_window), both ends included; (0, FS_ORDER_UNBOUNDED) = off.  It rides in the
    // directivity descriptor, by value with every launch
    int32_t min_order = 0, max_order = FS_ORDER_UNBOUNDED;
    bool windowed() const { return min_order != 0 || max_order != FS_ORDER_UNBOUNDED; }
    bool ext_connect() const { return d_dir != nullptr || windowed(); }   // its frames take the directional connect entries
    fs::Directivity directivity() const {
        fs::Directivity d;
        std::memcpy(d.fwd, fwd, sizeof(d.fwd)); d.samples = dir_samples; d.table = d_dir;
        d.min_order = min_order; d.max_order = max_order;
        return d;
    }
    // Two energy buffers [B][bins], alternating per frame: while the tail stream still reduces /
    // reconstructs frame f from one of them, the compute stream already traces frame f+1 into the other.
    float* d_energy[kEnergyBufs] = {};
    int cur = 0;                       // buffer of the current frame (rotates in fs_compute_energy_response*)
    hipEvent_t ev_dep = nullptr;       // compute stream: everything that writes the current buffer is enqueued
    hipEvent_t ev_rec[kEnergyBufs] = {};   // tail stream: the reconstruct that read buffer i is done
    bool rec_recorded[kEnergyBufs] = {};
    int last_rec = -1;                 // buffer the newest reconstruct read (its event also guards d_ir_*)
    hipEvent_t ev_rev = nullptr;       // reverb stream: the newest reverb callback has read d_ir_mono
    bool rev_recorded = false;
    // fs_reverb_process runs on the AUDIO thread while the game thread reconstructs: ir_mu guards what both touch —
    // last_rec / rec_recorded / ev_rec / ir_gen (written by the reconstruct, read by the callback) and rev_recorded / ev_rev
    // (the other way round).  Held only while work is ENQUEUED (microseconds), never across a stream wait.
    std::mutex ir_mu;
    uint64_t ir_gen = 0;               // bumped by every rewrite of the device IR (reconstructs, fs_set_impulse_response)
    float* energy() const { return d_energy[cur]; }
    // multi-GPU: the frame in the current buffer has been summed over the ranks (library collective), or handed to the
    // caller's collective (fs_energy_handoff); a world_size > 1 context refuses to reconstruct a frame that is neither
    bool reduced = false, handed_off = false;
    bool tail_ordered = false;         // the tail stream already waits for everything the compute stream wrote into the current buffer
    hipEvent_t ev_red[kEnergyBufs] = {};   // tail stream: the library's all-reduce of buffer i is done
    bool red_recorded[kEnergyBufs] = {};
    // deterministic mode (FS_FLAG_DETERMINISTIC): u64 fixed-point histograms [B][bins], allocated on first use,
    // alternating like the energy buffers; cur_fixed = the current frame deposited into d_fixed[cur]
    unsigned long long* d_fixed[kEnergyBufs] = {};
    bool cur_fixed = false;
    float* d_ir_bands = nullptr;  // [B + 1][samples]: the bands, then ...
    float* d_ir_mono = nullptr;   // ... (= d_ir_bands + B * samples) the channel view (all channels identical, FSAC.cpp:331)
    // newest publish that reads or writes the device IR set from the TAIL stream (a copy command behind reconstruct_now, a batch
    // kernel): a reconstruct on the compute stream waits for it before it writes the set.  0: none / a compute-stream publish.
    uint64_t cur_pub_seq = 0;
    uint64_t recon_sync_mark = ~0ull;    // fs_context::syncs at this source's last stand-alone reconstruct (fs_reconstruct_impulse_response_async)
    // ... and the other way round: the newest COMPUTE-stream launch that writes the set (its id in fs_context::h_pub_word; 0: none) —
    // a reconstruct on the tail stream lets the compute stream hand over first while that launch may still be running
    uint64_t dev_ir_word = 0;
    float* h_ir[kIrRing] = {};  // pinned host copies of the channel view
    int mask_index = -1;        // this source's row of fs_context::d_slot_masks (its handle; -1: none — every block is always written)
    hipEvent_t ev[kIrRing] = {};
    // How ring slot `slot` is known to be published, in this order: pub_word[slot] != 0 — a launch on the COMPUTE stream whose
    // reconstruct workgroups wrote the slot themselves and whose id appears in fs_context::h_pub_word (publish_arrive, fs_dev_recon.hpp:
    // no event, nothing on the tail stream); pub_batch[slot] != 0 — a batched reconstruct on the TAIL stream, one event for all its
    // sources (fs_context::tail_batch_ev); else the slot's own event ev[slot] behind a copy command on the tail stream.
    // rec_batch[i] != 0 names the tail batch whose event stands for ev_rec[i]; rec_on_compute[i]: the reconstruct ran on the compute
    // stream — nothing that stream does later needs to wait for it (ev_rec[i] is recorded only for a source with a reverb).
    uint64_t rec_batch[kEnergyBufs] = {};
    bool rec_on_compute[kEnergyBufs] = {};
    std::atomic<uint64_t> pub_word[kIrRing] = {};
    std::atomic<uint64_t> pub_batch[kIrRing] = {};
    std::atomic<uint64_t> seq_of[kIrRing] = {};   // (atomics: fs_get_impulse_response_sequence may look from another thread)
    std::atomic<uint64_t> enqueued{0};            // publishes enqueued so far
    std::atomic<uint64_t> front{0};    // newest COMPLETED publish (0 = none yet)
    // FS_FLAG_ROOM_PARAMETERS: the records of ring slot k are h_room[k * B .. (k + 1) * B) (pinned, allocated at the source's first
    // flagged reconstruct — ensure_room); room_of[k]: the publish in slot k carries them (noted with the slot's other notes)
    std::atomic<fs_room_parameters*> h_room{nullptr};
    std::atomic<bool> room_of[kIrRing] = {};
    // reverb (row f2): history rings [2][kReverbRing], write head (a callback's rows are staged in fs_context::rev_stage)
    float* d_ring = nullptr;
    unsigned rev_head = 0; int rev_frame = 0;
    // fs_reverb_set_engine: the engine the next fs_reverb_init gives the source / the one it was initialised with.  PARTITIONED
    // (fs_reverb_part.hip): d_ring is the engine's state block (ReverbPartItem: window history, products, delay line), float2
    // [part_state_elems]; N = 1 << part_n the transform, part_K partitions, part_slot the delay line's next slot;
    // d_fade_to / d_fade_from below are partition spectra [part_sets][part_K][N] float2, and d_fade_to exists without a fade length
    // too: every callback convolves its own spectra, taken like a crossfade's h_to (fade_primed, fade_gen).
    // part_sets: the spectrum sets of an IR copy — 1, with ears 2 (M_p, then S_p), a soundfield source's P = ceil(C / 2) channel pairs
    int32_t rev_engine_next = FS_REVERB_ENGINE_DIRECT, rev_engine = FS_REVERB_ENGINE_DIRECT;
    int part_n = 0, part_K = 0, part_slot = 0, part_sets = 0;
    // fs_reverb_set_ears: the choice for the next fs_reverb_init / what the source was initialised with.  With ears, the spectra are
    // taken from the band rows and the context's ear carriers of generation ear_gen.
    bool rev_ears_next = false, rev_ears = false;
    uint64_t ear_gen = 0;
    // fs_reverb_set_soundfield: likewise.  A soundfield source is a partitioned one whose d_ring is the state block of a mono row
    // with P products (P of the set installed at its init) and whose spectra are taken from the band rows and the context's
    // soundfield carriers of generation sf_gen
    bool rev_sf_next = false, rev_sf = false;
    uint64_t sf_gen = 0;
    // crossfade between successive IRs (fs_reverb_set_crossfade; the callback's own state, audio thread): fade_len L samples
    // (0: off), the callback's copies of the IRs it fades between (h_to = the newest it took, generation fade_gen),
    // fade_pos = samples output since the running fade began; fading == false: h_to alone is heard.
    // fade_primed == false: h_to holds nothing yet (after fs_reverb_init or enabling) — the next callback takes the IR unfaded.
    float* d_fade_from = nullptr; float* d_fade_to = nullptr;
    int32_t fade_len = 0, fade_pos = 0;
    bool fading = false, fade_primed = false;
    uint64_t fade_gen = 0;
    // direct sound (header: DirectRenderState, kDirectRenderHeader bytes), and the voice banks of the early reflections and of the
    // binaural voices.  br.r.taps = T; its rings were sized for T + H - 1 taps of the set in force at fs_binaural_render_init.
    // ar: the ambisonic voices' bank, with one ring and 128-byte slots (kAmbisonicBankHeader)
    RenderSetup dr;
    VoiceBank rr, br, ar;
    float occlusion = 1.0f;            // OcclusionAttenuation FSAC.h:130 (1.f until the first UpdateSound)
};
// The per-frame fields of a source switched to those of an EARLIER frame (energy buffer `cur`) for a scope: what a held frame or
// an owed reconstruct still has to do runs through code that works on "the source's current frame", while the source may have
// moved on to later frames (cur rotated).  At the end of the scope the fields come back — unless keep_if_current and the frame
// still is the source's current one: then what the scope did to it (reduced, handed over, ordered behind the tail) is its state.
struct SourceFrameScope {
    Source* const s;
    const int cur;
    const bool cur_fixed, reduced, handed_off, tail_ordered, restore;
    SourceFrameScope(Source* src, int frame_cur, bool fixed, bool frame_reduced, bool frame_tail_ordered, bool keep_if_current)
        : s(src), cur(src->cur), cur_fixed(src->cur_fixed), reduced(src->reduced), handed_off(src->handed_off),
          tail_ordered(src->tail_ordered), restore(!keep_if_current || src->cur != frame_cur) {
        s->cur = frame_cur; s->cur_fixed = fixed; s->reduced = frame_reduced; s->handed_off = false; s->tail_ordered = frame_tail_ordered;
    }
    ~SourceFrameScope() {
        if (restore) { s->cur = cur; s->cur_fixed = cur_fixed; s->reduced = reduced; s->handed_off = handed_off; s->tail_ordered = tail_ordered; }
    }
    SourceFrameScope(const SourceFrameScope&) = delete;
};

struct TimedFrame {
    hipEvent_t e[5];  // walk begin, walk end == connect begin, connect end | reconstruct begin, end
    bool has_trace = false, has_recon = false;
};

}  // namespace fsi
using namespace fsi;

// fs_scene_commit_progressive: the host's SAH build of a snapshot of the registered triangles, on its own thread, while
// the frames already trace through the device-built tree.  The thread touches nothing but this object.
struct RefineJob {
    std::vector<float> xyz; std::vector<uint16_t> mat; std::vector<uint32_t> obj;
    int T = 0;
    fs::HostBVH bvh;
    std::mutex mu; std::condition_variable cv;
    bool done = false;
    std::atomic<bool> cancel{false};   // a newer registration made this build useless: the builder gives up at its next check
};

// fs_scene_set_object_transforms (fs_capi_scene.cpp): everything the call keeps, allocated by the first call of a context.
// The REST pose (the positions last given by fs_scene_set_triangles / fs_scene_update_triangles) lives beside
// fs_context::h_xyz, which holds the WORLD positions; objects whose newest matrix h_xyz does not reflect yet are `stale`
// and brought up to date by sync_world_positions when a commit, the swap of a progressive commit or
// fs_scene_update_triangles needs them (the call itself does work proportional to the objects it lists).
struct ObjectMoves {
    static constexpr int kSets = 2;        // staging sets in rotation: a second call does not overwrite what the first one's kernel reads
    std::vector<float> rest;               // [T][9], input order (empty until the first call after fs_scene_set_triangles)
    double rest_amax = 0.0;                // largest |coordinate| the rest pose has held (grows only)
    // the objects' lists of input indices (CSR over h_obj), built at the first call after a commit; a slot = one object id
    bool lists_valid = false;
    std::unordered_map<uint32_t, uint32_t> slot_of;
    std::vector<uint32_t> off, idx;        // off [slots + 1] into idx [T]
    std::vector<float> m;                  // [slots][12]: the newest matrix of every stale object
    std::vector<uint8_t> stale;
    std::vector<uint32_t> stale_list, call_slots;
    std::vector<uint64_t> seen;            // the call that last listed the slot (an id twice in one call)
    uint64_t call = 0;
    // device copies of rest and idx, uploaded at the first call after a commit
    bool on_device = false;
    size_t dev_tris = 0;
    float* d_rest = nullptr;
    uint32_t* d_idx = nullptr;
    // bit pattern of the largest |coordinate| the kernel has written since the commit, and its pinned host copy
    uint32_t* d_amax = nullptr;
    uint32_t* h_amax = nullptr;
    hipEvent_t ev_amax = nullptr;
    bool amax_pending = false;             // a copy into h_amax is enqueued that fs_context::amax has not seen
    // per call: matrices [n][12] | prefix [n + 1] | start [n], pinned host block -> device block on the compute stream
    struct Set { char* h = nullptr; char* d = nullptr; hipEvent_t ev = nullptr; bool used = false; } set[kSets];
    size_t cap = 0;                        // objects per call the sets have room for
    int next = 0;
};

// A path query's staging pair (fs_capi_paths.cpp): pinned host memory and its device counterpart, both with room for `cap` rows.
// A buffer is a row of segments in the order of PathSegment, each [cap] times its bytes per row (0: the query has no such segment):
// the rows' sources as float4 | the counters a call clears, [cap] words each and side by side (a second-order query has two: near
// counters, then candidate counters) | near lists | candidate lists | confirmed records | what the copy back reads, rows [count]
// then paths [count][max_paths].  grow sizes the buffers and host / dev find a segment from the one PathLayout.
// Plain pointers: grow replaces the pair, release frees it (fs_context_destroy).
enum PathSegment { kSegSources, kSegCounters, kSegNear, kSegCand, kSegConf, kSegOut, kPathSegments };
struct PathLayout {
    size_t bytes_per_row[kPathSegments];
    size_t before(int seg) const {   // the bytes per row of the segments ahead of seg (kPathSegments: of them all)
        size_t sum = 0;
        for (int i = 0; i < seg; ++i) sum += bytes_per_row[i];
        return sum;
    }
};
struct PathStaging {
    char* h = nullptr;
    char* d = nullptr;
    int cap = 0;
    PathLayout pinned{}, device{};   // what grow was called with
    // room for `count` rows: a pair too small is replaced by one of twice the rows (32 at least) until it fits.  FS_OK or the failure reported.
    int grow(fs_context* ctx, int count, const PathLayout& pinned_layout, const PathLayout& device_layout);
    char* host(int seg) const { return h + (size_t)cap * pinned.before(seg); }
    char* dev(int seg) const { return d + (size_t)cap * device.before(seg); }
    size_t dev_bytes(int seg) const { return (size_t)cap * device.bytes_per_row[seg]; }
    void release();
};

// An audio callback's staging pair (fs_capi_reverb.cpp): pinned host memory and its device counterpart, in bytes.  What lies
// where is the call's CallbackLayout.  fit grows the pair: each side to the larger of what it has and what is asked, never
// smaller — the two sides do not grow in step when the count and the frame size vary apart, and a side that shrank would be
// reallocated by the next call of the old shape.  Plain pointers: fit replaces the pair, release frees it (fs_context_destroy).
struct CallbackStage {
    char* h = nullptr;
    char* d = nullptr;
    size_t host_cap = 0, dev_cap = 0;
    int fit(fs_context* ctx, size_t host_bytes, size_t dev_bytes);   // FS_OK or the failure reported
    void release();
};
// Where a callback of `count` rows of `frame` samples keeps what in its staging pair, every block 256-byte aligned.  What goes up in
// one copy has the same offsets on both sides: the call's own blocks (up[k], in the order given), then in [count][2 frame].  Behind
// it the host holds what comes back, out [count][row] | mix [row], row = the floats of an output row (2 frame; the ambisonic
// bus: C frame); the device holds the call's scratch blocks (scratch[k]), then out | mix, adjacent as on the host: one copy back.
struct CallbackLayout {
    size_t up[4] = {}, in = 0, up_bytes = 0;
    size_t h_out = 0, h_mix = 0, host_bytes = 0;
    size_t scratch[3] = {}, d_out = 0, d_mix = 0, dev_bytes = 0;
    size_t in_rows = 0;         // the bytes of in
    size_t rows = 0, row = 0;   // the bytes of out, and of mix
};

struct fs_context {
    fs_config cfg{};
    int num_bins = 0, num_samples = 0;
    hipStream_t stream = nullptr;
    // "tail" stream: [caller's all-reduce] -> reconstruct -> publish of frame f, concurrent with the tracing of
    // frame f+1 on `stream`
    hipStream_t copy_stream = nullptr;
    hipStream_t rev_stream = nullptr;  // the reverb callbacks' own stream (audio thread): never queued behind a traced frame
    bool own_stream = false;
    bool device_ok = false;
    std::string err;
    std::string advice;                // what fs_context_create found worth telling the host (fs_context_advice); never an error
    std::mutex err_mu;                 // the audio thread may fail too

    // scene (host staging + device)
    std::vector<float> h_xyz;
    std::vector<uint16_t> h_mat;
    std::vector<uint32_t> h_obj;   // actor id per triangle (empty = one actor per triangle)
    std::vector<float> h_absorption, h_transmission, h_scattering;
    int32_t T = 0, M = 0;
    bool committed = false;
    NodeQ4* d_nodes = nullptr;
    CoopChild* d_coop = nullptr;      // per-child records of the 4-wide nodes (fs_internal.hpp), rebuilt behind every commit and refit ...
    size_t coop_cap = 0;              // nodes it has room for
    CoopChild* d_coop16 = nullptr;    // ... and folded into the 16-wide nodes the cooperative traversal walks
    size_t coop16_cap = 0;
    int32_t* d_coop_levels = nullptr; // [2][kMaxBuildLevels + 2]: level_begin | dense index of every even level (uploaded at commit)
    int coop16_nodes = 0, coop_levels = 0;
    // the 48-byte node view of the chip-filling frame kernel (fs_internal.hpp: ViewRec), rebuilt behind every commit and refit
    ViewRec* d_view = nullptr;        // [nodes + triangles] node and triangle records, every node's children one block
    float4* d_view_nrm = nullptr;     // [nodes + triangles] unit normals of the triangle records
    uint32_t* d_view_scan = nullptr;  // [nodes + 1] records before each node's child block, less the root's (the layout: topology only)
    uint32_t* d_view_of_node = nullptr, *d_view_of_leaf = nullptr;   // node index / leaf-order position -> record
    uint32_t* d_view_bad = nullptr;   // raised by the fill: the tree cannot be restated (a step that is no power of two)
    size_t view_cap_nodes = 0, view_cap_tris = 0;
    bool view_ok = false;             // the committed scene has a view
    bool view_off = false;            // fs_debug_set_node_view(0): commits leave the scene without one (tests of the fallback)
    CoopInfo coop_info;               // what DeviceScene.coop_info points at
    float stage_margin = 1.3f;        // KParams.stage_margin
    DeepStore deep;                   // HBM spill area of the bounded LDS traversal stacks (DeviceScene.deep)
    int stack_rows_cap = kStackRowsCap;   // FS_STACK_ROWS_CAP
    Tri64* d_tris = nullptr;          // authoring records (builders, refit, fs_scene_update_triangles)
    Tri48* d_tris48 = nullptr;        // what the kernels traverse (fs_internal.hpp: Tri48), derived from d_tris
    float4* d_tri_nrm = nullptr;      // unit normals, leaf order
    float* d_absorption = nullptr;
    SoundAccum* d_sound = nullptr;
    // refit support (row f4, fs_refit.hip)
    uint32_t* d_leaf_pos = nullptr;   // input triangle -> leaf-order position
    float4* d_node_box = nullptr;     // [nodes][2] fp32 bounds scratch
    float* d_move = nullptr;          // staging for moved triangles
    size_t move_cap = 0;              // in triangles
    float amax = 0.f;                 // largest |coordinate| seen (sets the box padding)
    char* d_build = nullptr;          // fs_scene_commit_fast: device copies of the inputs + build scratch (grow-only)
    size_t build_cap = 0;
    size_t fast_cap_tris = 0;         // triangles the scene arrays of the last fast commit have room for (0: not reusable)
    bool refit_pending = false;
    ObjectMoves* moves = nullptr;     // fs_scene_set_object_transforms: null until its first call
    DeviceScene scene{};
    // ApplyMaterialFD work buffers (row f4), sized for the largest block seen
    int fft_n = -1;              // log2 of the size the twiddle table was built for
    int fft_cap_n = -1, fft_cap_l = 0;
    float2 *d_fft_x = nullptr, *d_fft_y = nullptr, *d_fft_w = nullptr;
    float *d_fft_in = nullptr, *d_fft_resp = nullptr, *d_fft_out = nullptr;
    // the 2 copies + up to 2 log2(N) - 20 launches of one block size are captured once into a hipGraph and replayed:
    // the sequence is launch-bound (16 launches for a 48 000-sample block)
    float* h_fft_stage = nullptr;      // pinned: in [L] | curves [3][bins] | out [3][L]
    size_t fft_stage_floats = 0;
    hipGraphExec_t fft_graph = nullptr;
    int fft_graph_n = -1, fft_graph_l = -1;
    // The audio callbacks' staging, one pair each, grown at the first call that needs more and freed with the context: a reverb, a
    // direct and a reflection callback of different counts may follow each other in one audio callback (and direct_stage below is
    // the game thread's).  Beside in, out and mix (CallbackLayout) they hold
    // rev_stage (fs_reverb_process / _batch): up, items [count] | the partitioned rows' items [count] | plain, fade, take lists of
    //   the two engines [6][count]; scratch, the mono tails cur [count][2 frame]
    // dr_stage (fs_direct_render_process_batch): up, items [count]; scratch, the plans [count]
    // rr_stage (fs_reflection_render_process_batch): up, items [count] | voices [count][stride]; scratch, the counters [count] |
    //   the plans [count][FS_MAX_REFLECTION_VOICES]
    // br_stage (fs_binaural_render_process_batch): up, items [count] | voices [count][stride] | the sounding slots' list; scratch,
    //   the counters [count] | the plans [count][FS_MAX_REFLECTION_VOICES] | the folded tables [sum of the rows' V][2][Tc], with a
    //   mesh in force followed by its wider plans and what the locate pass finds, [count][FS_MAX_REFLECTION_VOICES] each
    // ar_stage (fs_ambisonic_render_process_batch): rr_stage's blocks, with plans of 256 bytes and out [count][C frame] | mix [C frame]
    // sf_stage (fs_reverb_soundfield_process_batch): up, items [count] | plain, fade, take lists [3][count]; out [count][C frame] |
    //   mix [C frame]
    CallbackStage rev_stage, dr_stage, rr_stage, br_stage, ar_stage, sf_stage;
    // the HRIR set in force (fs_hrtf_set; the audio thread's): one device block, dirs [n][3] | hrir [n][2][H]; n == 0: none
    float* d_hrtf = nullptr;
    int hrtf_dirs = 0, hrtf_taps = 0;
    // ... the host's copy of its directions (what fs_hrtf_set_mesh validates against), and the mesh on it (fs_hrtf_set_mesh; dropped
    // by every fs_hrtf_set): one device block [m][3] float4 {row r_i of the triangle, the bits of its corner v_i}; m == 0: none
    std::vector<float> hrtf_dirs_host;
    float4* d_hrtf_mesh = nullptr;
    int hrtf_tris = 0;
    // ... and the onsets on it (fs_hrtf_set_onsets; dropped by every fs_hrtf_set, kept by fs_hrtf_set_mesh): one device block
    // [n][2] samples, the host's copy of the largest, and O = (int)omax + 1, the taps a delayed HRIR has beyond H; null and 0: none
    float* d_hrtf_onsets = nullptr;
    float hrtf_omax = 0.0f;
    int hrtf_onset_taps = 0;
    // the partitioned engine's twiddles, W[k] = exp(-2 pi i k / N), k < N / 2, per n = log2 N <= 12: built by the first
    // fs_reverb_init that needs the size, freed with the context
    float2* d_rev_tw[13] = {};
    // FS_FLAG_SPECTRAL_IR: the band edges (fs_set_band_edges: the B - 1 inner ones, ascending; empty = the defaults) and the
    // carriers built from them (fs_capi_publish.cpp: carrier_for — lazily, before the first spectral reconstruct)
    std::vector<double> band_edges;
    float* d_carrier = nullptr;          // [B][carrier_stride(num_samples)] fp32
    float carrier_build_ms = 0.0f;       // device time of the last build (HIP events)
    // fs_reverb_ears_set: the two-ear reverb's carrier set (null: none installed), what it was built from, and its generation —
    // bumped by every replacement, so that a source with ears takes again (Source::ear_gen)
    float* d_ear_carrier = nullptr;      // [2][B][carrier_stride(num_samples)] fp32: the mid rows cm_b, then the side rows cs_b
    float ear_radius_cm = 0.0f, ear_speed_cm_s = 0.0f;
    uint64_t ear_set_gen = 0;
    // fs_reverb_soundfield_set: the soundfield reverb's carrier set (null: none installed), its order, and its generation, bumped
    // by every replacement (Source::sf_gen)
    float* d_sf_carrier = nullptr;       // [C][B][carrier_stride(num_samples)] fp32, C = (sf_order + 1)^2
    int32_t sf_order = -1;
    uint64_t sf_set_gen = 0;
    // The path queries' staging (fs_capi_paths.cpp), one per query: the queries share no buffer.  Each is sized for its query's
    // largest max_paths, max_near and max_candidates, so that only a larger count grows it; its segments are the query's PathLayout.
    // direct_stage: the kernel reads the pinned sources in place.  d_direct_off: the sample-offset tables
    // [FS_MAX_DIRECT_SAMPLES][FS_MAX_DIRECT_SAMPLES][3] by n - 1, each uploaded at its first use.
    // diffract_f: the band centres f_b of the edges in force (diffract_f_edges, diffract_f_bands: what they were built from; rebuilt
    // when fs_set_band_edges has changed them), shared by the two diffraction queries.
    PathStaging direct_stage, reflect_stage, diffract_stage, reflect2_stage, diffract2_stage, mixed_stage, pathing_stage;
    // Pathing (fs_capi_paths.cpp): the probe set, its device block (allocated by the first fs_pathing_set_probes for
    // FS_MAX_PATHING_PROBES: probes | upper | graph | dL | d | pred, PathingSet of fs_internal.hpp) and the baked graph's host copy
    // [n][ceil(n / 32)].  scene_gen counts the commits, triangle updates, refits and object moves of the context; baked_gen is
    // its value at the bake: fs_pathing_info's scene_changed compares the two, nothing else reads them.
    struct Pathing {
        std::vector<float> xyz;
        char* d_block = nullptr;
        std::vector<uint32_t> graph;
        int32_t edges = 0;
        bool baked = false;
        uint64_t baked_gen = 0;
    } pathing;
    uint64_t scene_gen = 0;
    float* d_direct_off = nullptr;
    uint64_t direct_off_have = 0;
    double diffract_f[FS_MAX_BANDS] = {};
    std::vector<double> diffract_f_edges;
    int diffract_f_bands = 0;
    // the band-kernel tables fs_direct_render_init has built, one per (taps, edges in force); freed with the context
    struct DirectRenderTable { int taps; std::vector<double> edges; float* d; };
    std::vector<DirectRenderTable> dr_tables;
    HostBVH bvh;

    float listener[3] = {0, 0, 0};
    uint32_t listener_object = FS_NO_OBJECT;   // fs_listener_set_object
    std::vector<Source*> sources;

    // multi-GPU: RCCL communicator over the ranks that share the pairs of every frame
    ncclComm_t comm = nullptr;
    // cfg5 (independent sources, one per GPU): a communicator that never touches a frame — only fs_gather_energy uses it
    // fs_comm_enable_oneshot: the energy buffer's sum as one peer-write exchange instead of ncclAllReduce (fs_oneshot.hip)
    struct OneShot {
        bool on = false;
        OneShotView view{};
        void* own_mail = nullptr;         // this rank's mailbox (hipMalloc); the others are IPC mappings
        unsigned* d_err = nullptr;        // raised by a sum kernel that gave up waiting for a peer
        uint32_t seq = 0;                 // reduces issued so far
        bool broken = false;              // a sum gave up waiting for a peer: the sets are out of step, every later reduce is refused
    } oneshot;
    char* d_comm_stage = nullptr;         // 2 KB of device staging for the small collectives of fs_comm_enable_oneshot, allocated with the
                                          //   context: a rank that is out of memory later can still take part in them
    // One event per batched reconstruct launch on the tail stream, in a ring: the tail stream runs in order, so a batch is done as
    // soon as its own or ANY younger batch's event is (a batch whose ring entry has been recycled is covered by the oldest entry
    // still there).  Created with the context: the handles never change (the audio thread may query them).
    static constexpr int kTailBatches = 64;
    hipEvent_t tail_batch_ev[kTailBatches] = {};
    std::atomic<uint64_t> tail_batch_newest{0}, tail_batch_done{0};
    static constexpr int kReconTabSlots = 8, kReconTabItems = 256;
    ReconItem* h_recon_tab = nullptr;                  // pinned host: [kReconTabSlots][kReconTabItems], read by the batch kernel in place
    float** h_room_tab = nullptr;                      // ... and the parallel table of FS_FLAG_ROOM_PARAMETERS launches (allocated at the first)
    uint64_t recon_tab_batch[kReconTabSlots] = {};     // the tail-stream batch that last read slot k, or ...
    uint64_t recon_tab_word[kReconTabSlots] = {};      // ... the compute-stream launch (publish word id) that did
    unsigned recon_tab_next = 0;
    ncclComm_t peers = nullptr;
    int peers_size = 0;
    float* d_gather = nullptr; size_t gather_cap = 0;   // [peers][B][bins] fp32
    // Pipelined frames (fs_set_pipelining).  depth 1: the connect pass of frame f is held back and launched together with
    // the walk of frame f + 1 as ONE kernel; depth 2: the walk is held back as well — call f launches {plan of f, walk of
    // f - 1, connect of f - 2} as one kernel.  Anything that needs a held frame's result lets it finish alone (flush_pending).
    struct PipeFrame {
        WalkPart walk;               // its walk as the launchers take it: wl.rays_per_wave of its first stage; `stage` is set per launch
        ConnectPass connect;         // its connect pass (energy / fixed: the first item's buffers; a batched frame: the per-frame device
                                     //   tables — kBatchSlots of them rotate, a held frame is connected kMaxWalkParts + 1 calls later at most)
        std::vector<WalkStage> stages;    // the walk in one piece ({0, depth}) or the stages of a staged depth = 0 walk
        int next_stage = 0;          // stages [0, next_stage) have been launched; == stages.size(): only the connect pass is owed
        bool fixed = false;
        struct Item {                // one per source of the frame (a batched frame has several)
            Source* s = nullptr;
            int cur = 0;             // which of the source's energy buffers the frame deposits into
            bool want_recon = false; // fs_reconstruct_impulse_response_async arrived while the frame was held
            fs_params recon;
        };
        std::vector<Item> items;
    };
    std::deque<PipeFrame> held;
    // fs_set_frames_per_launch(n > 1): plain pipelinable frames are collected until n are waiting, then traced as ONE
    // batched frame in which every item keeps its own seed (and its own energy buffer, also for the same source twice) —
    // a 262 144-ray frame leaves a tenth of the chip idle that a launch of two such frames fills.  Everything that
    // flushes held frames dispatches a partial group first.
    struct GroupEntry {
        Source* s = nullptr; fs_params p; bool want_recon = false; fs_params recon;
        float pos[3] = {}, lis[3] = {};   // source and listener position AT THE CALL (either may move before the group is sent off)
        uint32_t object = FS_NO_OBJECT;
    };
    std::vector<GroupEntry> group;
    int frames_per_launch = 1;
    // Reconstructs that ride in the NEXT fused launch (single GPU): the frames the last launch connected owe their IR; a
    // reconstruct part behind the plan part produces it (fs_frame.hip) instead of a kernel on the tail stream that has to
    // squeeze into a chip the frame kernel fills (2 % of the frame kernel's time for 0.5 % of its work).  Everything that
    // flushes runs what is owed on the tail stream as before.  A frame that is not the source's last in the launch writes
    // its IR into a temporary buffer (two frames of one source would write the same d_ir_* at once) and is published from there.
    // reduced: the library has summed the buffer over the ranks on the tail stream (ev_red[cur]); such an entry rides in the
    // launch AFTER next (age >= 1 when a launch is assembled): the all-reduce runs behind the launch that connected the
    // frame, i.e. while the next one executes — a launch that waited for it would leave the GPU idle meanwhile
    struct ReconOwed { Source* s = nullptr; int cur = 0; bool fixed = false; fs_params p; bool reduced = false; int age = 0; };
    std::vector<ReconOwed> recon_owed;
    // Publishes of the compute stream (fused reconstruct parts, batches behind a tick or a flush): the launch writes the ring slots
    // and then its id into *h_pub_word (pinned, coherent) — see Source::pub_word.  pub_issued = id of the newest such launch.
    unsigned* d_pub_tickets = nullptr;             // device: the ticket cell of publish_arrive (re-armed by the launch that used it)
    // zero-block masks of the sources' host ring slots (fs_dev_recon.hpp: host_block_wanted): [kMaxMaskSources][kIrRing] words on the
    // device, bit b of word (source, slot) = block b of that slot may hold non-zero samples.  Kept by the reconstruct kernels; a
    // copy command into a slot (reconstruct_now, fs_set_impulse_response) sets the slot's word to all ones behind itself.
    uint32_t* d_slot_masks = nullptr;
    unsigned long long* h_pub_word = nullptr;
    uint64_t pub_issued = 0;
    int state_sets = 3;              // sets of the per-frame arrays (subpath state, records, schedules): frames in flight + 1
    bool state_cont = false;         // the sets include continuation records (staged walks)
    std::vector<int> stage_bounds;   // staged depth = 0 walks: the steps at which a walk changes launch (fs_set_walk_stages)
    bool stage_bounds_default = true; // not set by the host: grouped frames (two or more per launch) take kGroupedStageBounds
    std::vector<int> sync_stage_bounds;   // the same for depth = 0 frames that are waited for (stages back to back; FS_SYNC_WALK_STAGES)
    // the long-walk lane of such a frame (WalkLane): walks of sync_lane_len steps or more take cooperative waves of their
    // own from step 0 on, steps [0, sync_lane_end) beside the first stage, the rest beside the second (FS_SYNC_LANE: "len,end"; len 0: off)
    // -1 (default): by the frame's size and the roulette — sync_lane_plan, fs_capi_frame.cpp; with it the ONE default bound moves too
    int sync_lane_len = -1, sync_lane_end = 1 << 30;
    bool sync_stage_bounds_default = true;
    uint64_t syncs = 0;                   // fs_synchronize calls (a stand-alone reconstruct asks whether its producer waits for every frame: Source::recon_sync_mark)
    bool sync_stage_from_default = true;
    int sync_stage_from = 15000;          // ... of at least this many subpaths (smaller frames: every walk has a wave of its own anyway; with the long-walk lane an 8-source tick — 16 000 — gains 5 %, 14 000 lose: profiles/r05_stage_from.jsonl; 16 384 until then)
    std::shared_ptr<RefineJob> refine;   // fs_scene_commit_progressive: the background build whose tree replaces the device-built one
    std::vector<std::thread> refine_threads;   // every background build ever started (cancelled ones too): joined before the context goes
    bool moved_since_refine = false;     // fs_scene_update_triangles since the snapshot: re-apply the positions after the swap
    fs::HostBVH* prebuilt = nullptr;     // fs_scene_commit takes this tree instead of building one (install of a refined tree)
    int pipelining = 0;              // 0 off, 1 / 2 = frames held back
    unsigned frame_index = 0;        // consecutive traced frames rotate through the state / schedule / scratch sets
    size_t perm_words = 0;           // words of ONE schedule set (walk.perm holds state_sets)
    bool comm_owned = false;           // created by fs_comm_init (destroyed with the context) vs attached by the caller

    // subpath state (sized on demand)
    SubpathState st{};
    size_t cap_lanes = 0, cap_seg = 0;
    float4* d_seg_pos = nullptr;   // node positions per walk step, all-connections mode only (row f3)
    size_t cap_pos = 0;
    // second record tier of depth = 0 frames (walk steps beyond FS_MAX_DEPTH): [kOverLevels][over_cap] each, grown when
    // a frame raises the overflow word; d_overflow = that word
    float2* d_over_np = nullptr; uint32_t* d_over_mat = nullptr; float4* d_over_pos = nullptr;   // state_sets tiers each (positions: one)
    double* d_end_posd = nullptr; size_t cap_posd = 0;   // FS_FLAG_DOUBLE_POSITIONS: end points in double [lanes][3] (such frames are never held: one set)
    float4* d_cont = nullptr;        // continuation records of staged walks: [state_sets][2][cap_lanes]
    uint32_t over_cap = 0, over_cap_pos = 0;
    // FS_DEBUG_STALLS: where the producer waited (printed by fs_context_destroy): flushes of held frames, host waits for a publish
    // (count, microseconds), waits enqueued on the compute stream for another stream's event, owed reconstructs run on the tail stream
    bool debug_stalls = false;
    struct { uint64_t flushes = 0, flushed_frames = 0, sync_publish = 0, sync_publish_us = 0, waits_enqueued = 0, waits_skipped = 0, owed_on_tail = 0, launches = 0,
             tail_ops = 0, pub_word = 0, pub_event = 0, lane_launches = 0; } dbg;   // fs_get_pipeline_counters
    int over_cap_forced = 0;       // FS_OVER_CAP, read at fs_context_create
    unsigned* d_overflow = nullptr;   // the device's address of ...
    unsigned* h_overflow = nullptr;   // ... this pinned host word
    bool overflow_armed = false;   // an unbounded frame has been enqueued since the word was last read
    // batched frames (fs_compute_energy_response_batch_async): per-frame tables of pointers and source positions
    static constexpr int kBatchSlots = 2 * kMaxSets;   // frames the host may run ahead of the table copies (a held frame keeps its tables); >= the
                                                       //   launches after which the energy-buffer rotation of grouped frames repeats (24 / 2, 48 / 3, 48 / 4)
    char* d_batch = nullptr; char* h_batch = nullptr; size_t batch_cap = 0;   // kBatchSlots blocks of batch_cap bytes
    hipEvent_t ev_batch[kBatchSlots] = {};
    bool batch_pending[kBatchSlots] = {};
    size_t batch_bytes[kBatchSlots] = {};   // bytes of the table the slot's device copy holds (0: none) — same table again: no copy
    std::vector<char> batch_build;
    unsigned batch_frame = 0;
    // directivity tables replaced or dropped (fs_source_set_directivity): freed once the compute stream has passed the event
    // recorded at their retirement — every frame that may read one was enqueued on that stream before it
    struct RetiredTable { float* p; hipEvent_t ev; };
    std::vector<RetiredTable> retired_tables;
    unsigned long long host_segments = 0;   // walk segments of frames without a plan pass (roulette off), since the last reset

    // walk kernel launch shape (variant: FS_WALK_VARIANT in -DFS_EXPERIMENTS builds; coop: FS_WALK_COOP)
    WalkLaunch walk{2, 256, nullptr, nullptr};   // variant 2 = wave work sharing
    int hist_window = kHistWindow; // FS_HIST_WINDOW
    size_t lds_limit = 64 * 1024;  // dynamic LDS a workgroup may ask for on this device (hipDeviceAttributeMaxSharedMemoryPerBlock)
    int walk_rays_per_wave = 0;    // BDPT walk: subpaths per wave, 0 = by frame size (FS_WALK_RAYS_PER_WAVE; 64 = dense waves)

    // measurement
    int profiling = 0;   // 0 off, 1 = HIP events around the dominant (walk) kernel only, 2 = every kernel
    int profile_interval = 1;   // level 1: every n-th frame carries the events (fs_set_profiling_interval)
    unsigned profile_tick = 0;
    std::vector<TimedFrame> pending;
    std::vector<hipEvent_t> free_events;
    fs_stats stats{};

    int fail(int code, const std::string& m) {
        std::lock_guard<std::mutex> g(err_mu);
        err = m;
        return code;
    }
    int hip_fail(hipError_t e, const char* what) {
        std::lock_guard<std::mutex> g(err_mu);
        err = std::string(what) + ": " + hipGetErrorString(e);
        return FS_ERR_HIP;
    }
};

#define FS_FLUSH(ctx)                       \
    do {                                    \
        int fr_ = fsi::flush_pending(ctx);  \
        if (fr_) return fr_;                \
    } while (0)

#define FS_HIP(ctx, call)                                        \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return (ctx)->hip_fail(e_, #call); \
        if ((ctx)->deep.failed) {   /* a launcher could not grow the traversal stacks' deep store and skipped its launch */ \
            (ctx)->deep.failed = false;                          \
            return (ctx)->fail(FS_ERR_OUT_OF_MEMORY, "no device memory for the traversal stacks' deep store"); \
        }                                                        \
    } while (0)

#define FS_NCCL(ctx, call)                                               \
    do {                                                                 \
        ncclResult_t r_ = (call);                                        \
        if (r_ != ncclSuccess) return fsi::nccl_fail((ctx), r_, #call);  \
    } while (0)

constexpr float kMaxUnboundedRr = 0.95f;   // depth = 0 (uncapped walks): the strongest survival probability the record store covers

namespace fsi {

// ---- fs_capi_reverb.cpp: what the three audio callbacks share ------------------------------------------------------
// the layout of a call: out_row = the floats of an output row; up_blocks / scratch_blocks = the bytes of its own blocks
// (CallbackLayout::up / scratch), in order
CallbackLayout callback_layout(int count, int frame, size_t out_row, std::initializer_list<size_t> up_blocks,
                               std::initializer_list<size_t> scratch_blocks);
// The tail of a callback whose launches are enqueued on the reverb stream: the copy back (out | mix in one when both are wanted,
// else mix alone), the wait, mix copied out.  The rows of out are then in st.h + l.h_out: the caller's to copy.
int callback_finish(fs_context* ctx, const CallbackStage& st, const CallbackLayout& l, bool want_out, float* mix);
// ---- fs_capi_direct_render.cpp: what the voice bank's renderers share with the direct one (render_row: defined here) ----
bool direct_render_taps_ok(int32_t taps);
// What both inits do once the arguments are found good (need = d_max + taps + 1 + frame samples, the ring's least size): the
// table of (taps, edges in force), the wait for the callbacks' stream, the old state block freed, a zeroed new one of
// header bytes + the `rings` rings.  A failure before the wait changes nothing; one after it leaves the source without a set-up.
int render_setup(fs_context* ctx, RenderSetup& r, size_t header, int rings, int frame, int taps, double d_max, double need);
int render_clear(fs_context* ctx, const RenderSetup& r, size_t header, int rings);   // the releases: history := 0 (enqueued), where there is a set-up
// a row's first checks, in this order: the handle, the set-up (which(source): the one of the source's three that the callback
// renders with; no_setup: the message), the batch's one shape (first: row 0's source, nullptr in row 0).  *rc = FS_OK and the
// source, or the failure reported and nullptr.
Source* get_source(fs_context* ctx, fs_source h);   // (fs_capi_context.cpp)
template <typename Which>
Source* render_row(fs_context* ctx, fs_source h, Which&& which, const char* no_setup, const Source* first, int* rc) {
    Source* s = get_source(ctx, h);
    if (!s) *rc = ctx->fail(FS_ERR_BAD_HANDLE, "bad source handle");
    else if (!which(*s).d) *rc = ctx->fail(FS_ERR_INVALID_ARGUMENT, no_setup);
    else if (first && (which(*s).frame != which(*first).frame || which(*s).taps != which(*first).taps))
        *rc = ctx->fail(FS_ERR_INVALID_ARGUMENT, "the sources of a batch share one frame size and one tap count");
    else *rc = FS_OK;
    return *rc ? nullptr : s;
}
// a target's or a voice's (`whose`) delay and band gains against the source's set-up
int render_aim_check(fs_context* ctx, const char* whose, float delay, const float* band_gain, const RenderSetup& r);
int render_no_duplicates(fs_context* ctx, const std::vector<Source*>& srcs);   // "a source appears twice in the batch"
// ---- fs_capi_reflect_render.cpp: the voice bank's host side, the reflection and the binaural renderer's alike ----------
// (the callback itself is fs_capi_voice_bank.hpp's voice_bank_process)
// what one row's matching decides: the slots' ops (kVoiceIdle ...), the slot table afterwards, the counts
struct VoiceMatch {
    int8_t op[FS_MAX_REFLECTION_VOICES];
    bool held[FS_MAX_REFLECTION_VOICES];
    uint32_t key[FS_MAX_REFLECTION_VOICES];
    fs_reflection_render_row row;
};
// rule 1 of the reflection renderer on a source's slot table: `voices` = the row's n entries, voice_bytes apart, each beginning
// with its key
VoiceMatch voice_match(const VoiceBank& bank, const void* voices, size_t voice_bytes, int n);
// What fs_reflection_render_init, fs_binaural_render_init and fs_ambisonic_render_init do with their arguments: `which` = the
// source's bank; fold_taps = the taps a voice's filter grows by (H - 1 of the set in force; 0: none), a negative one = no set in
// force; the texts are the entry point's own refusals: no set, the arguments' ranges, too many folded taps, too long a history;
// header, rings = the bytes of the bank's header and the number of history rings behind it.
struct VoiceBankInitTexts { const char *no_set, *ranges, *folded, *ring; };
int voice_bank_init(fs_context* ctx, fs_source h, VoiceBank Source::*which, int fold_taps, const VoiceBankInitTexts& t, int32_t frame_size,
                    int32_t taps, int32_t voices, float max_delay_seconds, size_t header, int rings);
int voice_bank_release(fs_context* ctx, fs_source h, VoiceBank Source::*which, size_t header, int rings);   // history := 0, every slot free
// ---- fs_capi_context.cpp ------------------------------------------------------------------------------------------
Source* get_source(fs_context* ctx, fs_source h);
hipError_t wait_energy_readers(fs_context* ctx, Source* s);            // before the compute stream writes the current energy buffer
hipError_t compute_waits_for(fs_context* ctx, hipEvent_t ev);   // hipStreamWaitEvent on the compute stream unless ev has completed
hipError_t wait_energy_readers(fs_context* ctx, Source* s, int buf);   // ... or the buffer the next frame will use
hipError_t handoff_energy(fs_context* ctx, Source* s);        // compute stream -> tail stream
void free_source(fs_context* ctx, Source* s);
void free_scene(fs_context* ctx);
void free_object_moves(fs_context* ctx);   // fs_capi_scene.cpp (the caller has synchronised the compute stream)
void free_state(fs_context* ctx);
hipEvent_t take_event(fs_context* ctx);
void resolve_timings(fs_context* ctx);
void resolve_completed_timings(fs_context* ctx);
void poll_published(fs_context* ctx, Source* s);
bool tail_batch_done(fs_context* ctx, uint64_t id);                 // any thread
hipEvent_t tail_batch_event(fs_context* ctx, uint64_t id);          // the event that covers batch `id`
hipError_t stream_waits_for_rec(fs_context* ctx, hipStream_t st, Source* s, int buf);   // st waits for the reconstruct that last read energy buffer `buf` (and wrote d_ir_*)
hipError_t wait_event_polling(hipEvent_t ev);   // short producer waits: poll, do not sleep (fs_capi_context.cpp)
bool pub_word_done(const fs_context* ctx, uint64_t id);             // any thread: has compute-stream publish `id` reached the host word?
hipError_t wait_pub_word(fs_context* ctx, uint64_t id);             // producer: poll the host word (falls back to a stream wait)
PublishWord next_pub_word(fs_context* ctx);                         // the arguments of the next self-publishing launch (id = pub_issued + 1; commit with ++pub_issued)
bool slot_published(fs_context* ctx, Source* s, int slot);          // any thread: the publish in ring slot `slot` has completed
uint32_t* slot_mask_ptr(const fs_context* ctx, const Source* s, int slot);   // the slot's zero-block mask word on the device (nullptr: none)
hipError_t slot_mask_all_dirty(fs_context* ctx, const Source* s, int slot, hipStream_t st);   // behind a copy command into the slot
hipError_t sync_publish(fs_context* ctx, Source* s, int slot);      // block until the publish in ring slot `slot` has completed
int ensure_state(fs_context* ctx, uint32_t n_local, int levels, bool unbounded, double rr_prob, bool want_positions, bool want_normals,
                 int sets, bool staged);
int auto_rays_per_wave(unsigned long long lanes, int depth, unsigned long long waves = 0);
int auto_pairs_per_wave(unsigned long long pairs);
int check_params(fs_context* ctx, const fs_params* p);
// FS_FLAG_SPECTRAL_IR: can this context build its carriers (K within the FFT, every band at least one bin under Nyquist)?
// edges: the B - 1 inner edges to check (nullptr: the context's own, or the defaults).  FS_OK, or the failure reported.
int check_band_edges(fs_context* ctx, const double* edges, const char* what);
int check_spectral(fs_context* ctx, const fs_params* p);
// the carrier set a reconstruct with these params uses: nullptr without FS_FLAG_SPECTRAL_IR; built (and waited for) on first use
int carrier_for(fs_context* ctx, const fs_params* p, const float** out);
// W[k] = exp(-2 pi i k / N), k < N / 2, computed in double: the twiddle table of every N-point transform (N a power of two; N < 2: [1])
std::vector<float2> host_twiddles(size_t N);
// fs_reverb_ears_set's build for the band edges in force: a new [2][B][carrier_stride] set on the compute stream, waited for
int build_ear_carriers(fs_context* ctx, float radius_cm, float speed_cm_s, const char* what, float** out);
// ... and its installation in place of the one in force (nullptr: none), behind the reverb stream
int install_ear_carriers(fs_context* ctx, float* set, float radius_cm, float speed_cm_s);
// fs_reverb_soundfield_set's build for the band edges in force, a new [C][B][carrier_stride] set of C = (order + 1)^2 channels, and
// its installation (nullptr: none, order -1), under the same two contracts
int build_soundfield_carriers(fs_context* ctx, int32_t order, const char* what, float** out);
int install_soundfield_carriers(fs_context* ctx, float* set, int32_t order);

// ---- fs_capi_scene.cpp --------------------------------------------------------------------------------------------
// fs_scene_commit_progressive: swap the finished background tree in; drop / wait for a background build
int maybe_install_refined(fs_context* ctx);
void cancel_refine(fs_context* ctx);
void wait_refine(const std::shared_ptr<RefineJob>& j);
void join_refine_threads(fs_context* ctx);

// ---- fs_capi_frame.cpp --------------------------------------------------------------------------------------------
int dispatch_group(fs_context* ctx);         // the frames collected by fs_set_frames_per_launch as ONE batched frame

// ---- fs_capi_pipeline.cpp -----------------------------------------------------------------------------------------
int flush_pending(fs_context* ctx);          // pipelined frames: drain the pipeline (fused launches, or every held frame on its own kernels)
int check_overflow(fs_context* ctx);         // depth = 0: did a record miss both tiers?  (stream just synchronised)
// what a held frame still owes once its connect pass has been enqueued (fixed-point rounding, the sum over the ranks, its reconstruct)
int finish_held_frame(fs_context* ctx, const fs_context::PipeFrame& q, bool may_defer_recon = false, bool draining = false);
// One fused-launch round: the parts the caller has preset in `fp` (the frame call: its plan part; the drain: nothing), the next
// walk stage of every held frame, the connect pass of the oldest complete one and the owed reconstructs as ONE launch, and what
// follows it (the publishes, the stages advanced, the connected frame finished).  end_event: a timed frame's second event,
// recorded right behind the launch if it carried a walk and a connect part.
struct RoundCarried { bool any = false, walk = false, connect = false; };   // any == false: there was nothing a launch could carry
int fused_round(fs_context* ctx, FrameParts& fp, bool draining, hipEvent_t end_event, RoundCarried* carried);

// ---- fs_capi_publish.cpp ------------------------------------------------------------------------------------------
// The reconstruct parts of a fused launch: owed_prepare turns the owed reconstructs into parts of the launch being assembled (and
// takes their sources' IR mutexes), owed_publish notes the publishes behind the launch (which announces them itself).
struct OwedLaunch {
    std::vector<fs_context::ReconOwed> owed;
    std::vector<uint64_t> seq;                             // publish number of each entry (ring slot = seq % kIrRing)
    std::vector<char> newest;                              // the source's newest frame of the launch: its IR becomes the device-resident set
    std::vector<std::unique_lock<std::mutex>> locks;
    PublishWord pub;
    unsigned tab_slot = 0;                                 // the slot of fs_context::h_recon_tab that holds the launch's items
};
int owed_prepare(fs_context* ctx, FrameParts& fp, OwedLaunch& ol);
int owed_publish(fs_context* ctx, OwedLaunch& ol, bool launched_fused);
int run_owed_reconstructs(fs_context* ctx);  // the reconstructs that were waiting for the next fused launch, on kernels of their own after all
int flush_reconstruct(fs_context* ctx, Source* s, const fs_params* p);   // a reconstruct no launch is fused with (one GPU: a compute-stream batch of one)
int reconstruct_now(fs_context* ctx, Source* s, const fs_params* p);
int reconstruct_batch(fs_context* ctx, Source* const* srcs, int count, const fs_params* p, bool on_compute);   // many sources: one launch, one event
int ir_ring_backpressure(fs_context* ctx, Source* s, int more);   // the IR ring's throttle before `more` publishes (may block; not under ir_mu)
int ir_ring_backpressure_for(fs_context* ctx, Source* s);
hipError_t tail_waits_for_compute_ir(fs_context* ctx, Source* s);   // before the tail stream writes the source's device IR set
int ensure_room(fs_context* ctx, Source* s);   // FS_FLAG_ROOM_PARAMETERS: the source's record ring (and the context's batch table)

// ---- fs_capi_comm.cpp ---------------------------------------------------------------------------------------------
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;   // why loading failed
};
RcclApi* rccl();   // nullptr: librccl is not loadable
int nccl_fail(fs_context* ctx, ncclResult_t r, const char* what);
int reduce_energy(fs_context* ctx, Source* s);   // sum the source's current energy buffer over the ranks (tail stream)
void oneshot_release(fs_context* ctx);
int oneshot_check(fs_context* ctx);             // FS_ERR_COMM if a one-shot sum gave up waiting (tail stream synchronised)

}  // namespace fsi
