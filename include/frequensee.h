/*
 * frequensee.h — C ABI of the MI355X-native FrequenSee acoustic BDPT path.
 *
 * Drop-in boundary for the per-frame bidirectional path trace + energy-buffer loop of the
 * FrequenSee Unreal plugin (henreedev/audio-pathtracer).  Every entry point names the reference
 * interface it replaces; paths are relative to Plugins/FrequenSee/Source/FrequenSee/ in the
 * reference tree:
 *   ARTS.h/.cpp = Public/AudioRayTracingSubsystem.h, Private/AudioRayTracingSubsystem.cpp
 *   FSAC.h/.cpp = Public/FrequenSeeAudioComponent.h, Private/FrequenSeeAudioComponent.cpp
 *   MAT.h, GEO.h = Public/AcousticMaterial.h, Public/AcousticGeometryComponent.h
 *
 * Conventions: extern "C", POD only, every call returns an int status (FS_OK == 0), no exception
 * crosses the boundary, output buffers are caller-allocated, handles are opaque.  Positions are
 * Unreal units (cm).  One context drives one HIP device.  Its tracing is ordered on one HIP stream (the
 * "compute" stream: its own, or the caller's via fs_config.stream).  On one GPU the reconstruct and the publish of
 * the impulse response ride on that stream too: the reconstruct workgroups write the pinned host ring slot themselves
 * and announce it in a pinned host word — no second queue, no copy command, no event in the steady state of a stream
 * of frames.  The context's second ("tail") stream carries what has to run beside the tracing: a multi-GPU reduce
 * (the library's or a caller's behind fs_energy_handoff) with the reconstruct of such a frame, and the few reconstructs
 * with per-kernel timing or a literal second flush.  A context is not re-entrant:
 * one producer thread (the game thread) calls compute/reconstruct; concurrently with it any number of threads may
 * read published impulse responses (fs_get_impulse_response), and ONE audio render thread may run the reverb callback
 * (fs_reverb_process) — it has a HIP stream of its own and is never queued behind a traced frame.
 * The tail stream and the reverb stream are created with the highest HIP stream priority (small work somebody waits for;
 * priority streams have hardware queues of their own).
 *
 * There is no CPU fallback: if no HIP device is usable every compute entry point fails with
 * FS_ERR_NO_DEVICE.
 *
 * TWO TIERS.  CORE = the drop-in boundary itself: what a UE shim inside UpdateSource / TickComponent
 * binds, and nothing a host has to know beyond the reference's own interface —
 *   CORE:     fs_abi_version fs_config_default fs_params_default fs_context_create fs_context_destroy fs_last_error
 *             fs_scene_set_triangles fs_scene_set_materials fs_scene_set_objects fs_scene_commit
 *             fs_source_create fs_source_destroy fs_source_set_position fs_source_set_object
 *             fs_listener_set_position fs_listener_set_object
 *             fs_compute_energy_response fs_reconstruct_impulse_response fs_update_sources
 *             fs_get_impulse_response fs_copy_impulse_response fs_get_impulse_response_sequence
 *             fs_get_energy_buffer fs_flush_energy_buffer fs_add_energy_at_delay fs_update_energy_buffer
 *             fs_num_bins fs_num_samples fs_get_occlusion_attenuation fs_update_sound fs_sound_params_default
 *             fs_get_stats fs_reset_stats
 * EXTENDED = everything else: the asynchronous / batched / pipelined forms of the two hot calls, multi-GPU plumbing,
 * run-time scene changes, the rows SURVEY.md 8(f) ranks next (text interchange, reverb, material filter), measurement
 * and tools.  A host can ignore all of it and still be correct; it is there for throughput and for the tests —
 *   EXTENDED: fs_context_advice fs_scene_commit_fast fs_scene_commit_progressive fs_scene_refine_pending
 *             fs_scene_refine_wait fs_scene_update_triangles fs_scene_refit fs_scene_set_object_transforms
 *             fs_compute_energy_response_async fs_compute_energy_response_batch_async
 *             fs_reconstruct_impulse_response_async fs_reconstruct_impulse_response_batch_async fs_synchronize fs_submit
 *             fs_set_pipelining fs_set_walk_stages fs_set_frames_per_launch fs_set_band_edges
 *             fs_energy_device_ptr fs_energy_handoff fs_shard_range fs_comm_unique_id fs_comm_init fs_comm_attach
 *             fs_comm_enable_oneshot fs_comm_detach fs_comm_info fs_peers_init fs_peers_detach fs_gather_energy fs_gather_energy_async
 *             fs_copy_band_impulse_response fs_set_impulse_response fs_trace_rays
 *             fs_save_array_to_file fs_load_float_array fs_save_impulse_response
 *             fs_reverb_init fs_reverb_process fs_reverb_process_batch fs_reverb_release fs_reverb_set_crossfade fs_reverb_set_engine fs_apply_material_fd
 *             fs_reverb_ears_default fs_reverb_ears_set fs_reverb_ears_info fs_reverb_set_ears fs_reverb_copy_ear_impulse_responses
 *             fs_reverb_soundfield_set fs_reverb_soundfield_info fs_reverb_set_soundfield
 *             fs_reverb_copy_soundfield_impulse_responses fs_reverb_soundfield_process_batch
 *             fs_set_profiling fs_set_profiling_interval fs_get_pipeline_counters fs_get_streams
 *             fs_source_set_orientation fs_source_set_directivity fs_get_room_parameters
 *             fs_source_set_order_window fs_source_get_order_window
 *             fs_direct_params_default fs_direct_sample_offsets fs_update_direct_paths
 *             fs_reflection_params_default fs_update_reflection_paths
 *             fs_diffraction_params_default fs_update_diffraction_paths
 *             fs_reflection2_params_default fs_update_reflection2_paths
 *             fs_diffraction2_params_default fs_update_diffraction2_paths
 *             fs_mixed_params_default fs_update_mixed_paths
 *             fs_pathing_set_probes fs_pathing_bake_params_default fs_pathing_bake fs_pathing_info fs_pathing_copy_graph
 *             fs_pathing_params_default fs_update_pathing_paths
 *             fs_direct_band_kernels fs_direct_render_init fs_direct_render_release fs_direct_render_process_batch
 *             fs_reflection_render_init fs_reflection_render_release fs_reflection_render_process_batch
 *             fs_hrtf_set fs_hrtf_info fs_hrtf_spherical_head
 *             fs_hrtf_triangulate fs_hrtf_mesh_rows fs_hrtf_mesh_locate fs_hrtf_set_mesh fs_hrtf_mesh_info
 *             fs_hrtf_set_onsets fs_hrtf_onsets_info fs_hrtf_delay fs_hrtf_split_onsets fs_hrtf_spherical_head_split
 *             fs_binaural_render_init fs_binaural_render_release fs_binaural_render_process_batch
 *             fs_ambisonic_encode fs_ambisonic_render_init fs_ambisonic_render_release fs_ambisonic_render_process_batch
 * (tests/test_capi_cpu.py checks that every exported symbol is in exactly one of the two lists.)
 * Environment variables (FS_*) are tuning and diagnostic knobs only; all of them are read ONCE — at fs_context_create, at a
 * scene commit (builder knobs) or at the first launch of a kernel family — never per frame.
 */
#ifndef FREQUENSEE_H
#define FREQUENSEE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(FS_BUILDING_LIBRARY) && defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: only this header is exported */
#endif

#define FS_ABI_VERSION 5
#define FS_MAX_BANDS 8
#define FS_NO_MATERIAL 0xFFFFu /* actor without UAcousticGeometryComponent / Material (ARTS.cpp:383) */
#define FS_MAX_DEPTH 64        /* largest explicit depth cap.  depth == 0 means NO cap, like the reference's while (true)
                                * (ARTS.cpp:294): a walk ends when the roulette ends it (without roulette, or with
                                * rr_prob >= 1, depth == 0 means FS_MAX_DEPTH) */

/* status codes (replace the reference's check()/UE_LOG error behaviour) */
enum {
    FS_OK = 0,
    FS_ERR_INVALID_ARGUMENT = 1,
    FS_ERR_NO_DEVICE = 2,     /* no usable HIP device / HIP runtime error at init */
    FS_ERR_HIP = 3,           /* a HIP call failed; fs_last_error() has the text */
    FS_ERR_NOT_COMMITTED = 4, /* scene not committed */
    FS_ERR_BAD_HANDLE = 5,
    FS_ERR_SIZE_MISMATCH = 6, /* UpdateEnergyBuffer's check(Num()==NumBins), FSAC.h:83 */
    FS_ERR_OUT_OF_MEMORY = 7,
    FS_ERR_COMM = 8,          /* multi-GPU: librccl not loadable, an RCCL call failed, or a sharded frame was not reduced */
    FS_ERR_OVERFLOW = 9       /* depth = 0 only: more walks than provisioned outlived FS_MAX_DEPTH steps; the library has grown
                               * its record store — trace the frame again (fs_compute_energy_response does so by itself,
                               * the _async entry points report it at the next fs_synchronize) */
};

/* compat flags: reproduce a reference quirk literally (default 0 = evident intent) */
#define FS_FLAG_FIXED_NORM_1000 1u          /* ARTS.cpp:164 normaliser 1/USED_RAY_COUNT whatever NumRays is */
#define FS_FLAG_FLUSH_BEFORE_RECONSTRUCT 2u /* build-owned: what ARTS.cpp:191 would do if FlushEnergyBuffer zeroed the buffer as its name
                                             * and comment say (FSAC.h:76-79) — the IR becomes all zero.  At HEAD it does NOT:
                                             * TArray::SetNumZeroed only zero-fills elements it ADDS, so after the first call
                                             * both flushes are no-ops; the literal behaviour is FS_FLAG_ACCUMULATE_ENERGY */
#define FS_FLAG_ACCUMULATE_ENERGY 128u      /* HEAD literally: EnergyBuffer.SetNumZeroed(NumBins) (FSAC.h:78) keeps the old values,
                                             * so the deposits of every UpdateSource add to those of all earlier ones (the
                                             * "energy accumulation" the reference's README lists as a known bug).  The frame
                                             * deposits into the buffer the previous frame of this source used, without clearing it
                                             * (single-GPU contexts only; with FS_FLAG_DETERMINISTIC the fixed-point histogram
                                             * accumulates — keep one mode for the whole accumulation) */
#define FS_FLAG_COSINE_SAMPLING 4u          /* cosine-weighted bounce instead of VRandCone(n, 90 deg).  Both maps build the direction in the
                                             * tangent frame of Duff et al. 2017, which reads copysign(1, n.z) — the sign of a ZERO too: off
                                             * a wall with n.z = 0 the bounce depends on whether the hit normal's zero is +0 (the triangle's
                                             * winding normal e1 x e2) or -0 (that normal negated, zeros included, because it faced along
                                             * the ray).  DESIGN.md section 4 has the formulas. */
#define FS_FLAG_ALL_CONNECTIONS 16u         /* row f3, the reference's unfinished draft (Is_NaiveConnections, ARTS.cpp:518-546): connect every
                                             * forward prefix F0..Fi with every backward prefix B0..Bj of a pair (visibility test and
                                             * EvaluatePath as for the end-to-end connection) and combine the (i, j) that give the same
                                             * path length with uniform weights 1/N(i+j); ~(k+1)(m+1) contributions per pair instead of 1 */
#define FS_FLAG_MIS_BALANCE 32u             /* row f3: balance-heuristic weights for the all-connections mode (implies it) — the intent of
                                             * the draft's MISEnergy / getExpectedWeight, ARTS.cpp:548-597 ("the weight considers other
                                             * strategies that could have produced the same path"): weight of the (i, j) that produced a
                                             * path = its sampling density / the sum over all (i', j') of the same path length, with the
                                             * densities the walk uses (1/4pi at the end points, CosTheta/PI at surfaces, ARTS.cpp:306-318)
                                             * in area measure; uniform weight when a segment is degenerate */
#define FS_FLAG_MATERIAL_LOBES 64u          /* row f4: a walk vertex reached by a hit picks ONE of three lobes from the material's
                                             * Absorption / Transmission / Scattering arrays (MAT.h:22-30), split as ApplyMaterialFD does
                                             * per bin (MaterialAcousticProcessor.cpp:51-72: Refl = 1 - alpha, tau clamped to Refl + tau
                                             * <= 1, specular Refl (1 - sigma), diffuse Refl sigma, transmitted tau): diffuse = the
                                             * reference's cone sample, specular = mirror direction, transmitted = straight on from the
                                             * far side; EvaluatePath then uses that lobe's gain (diffuse / pi at a connection vertex)
                                             * instead of Absorption / pi.  The reference's walk is diffuse only ("FIXME assuming
                                             * diffuse", ARTS.cpp:304).  Not combinable with FS_FLAG_MIS_BALANCE. */
#define FS_FLAG_DOUBLE_POSITIONS 256u       /* node positions in double like the reference's FVector (ARTS.h:61): hit point, surface
                                             * offset, subpath end points, the connection ray's direction and length and every
                                             * segment length are computed in double and narrowed where the reference narrows them
                                             * (FVector::Dist(...) / 1000.f assigned to a float, ARTS.cpp:372-373); the line trace itself
                                             * starts from the float-rounded node as before.  Bit-for-bit the oracle's double-position
                                             * build (oracle/Makefile target dpos).  Costs a few % of the walk; such frames are never
                                             * held by fs_set_pipelining.  Not combinable with the lobe / all-connections modes. */
#define FS_FLAG_SPECTRAL_IR 512u           /* read by the RECONSTRUCT calls (fs_reconstruct_impulse_response[_async], _batch_async,
                                             * fs_update_sources): the channel view becomes a broadband IR whose spectrum follows the
                                             * per-band energies, y[n] = (1/sqrt(B)) sum_b env_b[n] c_b[n] — env_b = band row b (unchanged,
                                             * fs_copy_band_impulse_response), c_b = band-limited noise of unit mean square: the real part
                                             * of the inverse FFT (K = next power of two >= fs_num_samples) of the band's bins with unit
                                             * magnitude and phase 2 pi (splitmix64(0x5EED + k) >> 40) 2^-24.  Bands: the crossovers of
                                             * fs_set_band_edges, by default octaves centred at 125, 250, ... Hz (edges 125 * 2^(b - 0.5)).
                                             * Every consumer of the channel view (ring, reverb, export) gets it.  Rejected when the
                                             * edges do not fit under sample_rate / 2.  The carriers are built once per context. */
#define FS_FLAG_ROOM_PARAMETERS 1024u      /* read by the RECONSTRUCT calls (fs_reconstruct_impulse_response[_async], _batch_async,
                                             * fs_update_sources): the launch that reconstructs and publishes the IR also computes the
                                             * room parameters of each band's histogram (fs_room_parameters) and publishes them under the
                                             * same publish number — fs_get_room_parameters.  Such a reconstruct never rides in a fused
                                             * launch of held frames (fs_set_pipelining): it runs on a kernel of its own. */
#define FS_FLAG_DETERMINISTIC 8u            /* deposits are summed as 64-bit integers of 2^-40 energy quanta: the
                                             * histogram no longer depends on the order of the atomics, so it is bit-identical
                                             * from run to run and for every split of the pairs over GPUs (sum-reduce the u64
                                             * buffer fs_energy_handoff returns; it is rounded to fp32 once, after the reduce) */

typedef struct fs_context fs_context;
typedef int32_t fs_source; /* handle of one registered UFrequenSeeAudioComponent */

/* Subsystem/component sizing constants (FSAC.h:133-139). Zero fields take the reference value. */
typedef struct fs_config {
    uint32_t struct_size;      /* = sizeof(fs_config) */
    int32_t device;            /* HIP device ordinal */
    int32_t num_bands;         /* B, 1..FS_MAX_BANDS; 1 = the reference (band slot 0 == Absorption[2]) */
    int32_t sample_rate;       /* 48000  FSAC.h:133 */
    int32_t num_channels;      /* 2      FSAC.h:135 */
    float simulated_duration;  /* 1.0 s  FSAC.h:136 */
    float bin_duration;        /* 0.001 s FSAC.h:137 */
    int32_t rank;              /* multi-GPU: this process traces pairs [rank*P/W, (rank+1)*P/W) */
    int32_t world_size;        /* W >= 1 */
    void* stream;              /* optional hipStream_t owned by the caller (e.g. the harness's); NULL = own stream */
} fs_config;

/* Per-update parameters; defaults (fs_params_default) are the constants compiled into the reference. */
typedef struct fs_params {
    uint32_t struct_size;      /* = sizeof(fs_params) */
    uint32_t flags;            /* FS_FLAG_* */
    uint64_t seed;             /* counter-based RNG key (replaces the global rand() behind FMath::FRand) */
    uint32_t num_rays;         /* R = source + listener subpaths per frame over all ranks; pairs P = R/2.
                                  reference: NumRays = USED_RAY_COUNT = 1000 pairs = 2000 (ARTS.h:176) */
    int32_t depth;             /* max segments per subpath, 1..FS_MAX_DEPTH; 0 = unbounded like ARTS.cpp:294 */
    int32_t russian_roulette;  /* 1 = ARTS.cpp:300-301 */
    float rr_prob;             /* 0.9       ARTS.cpp:282 */
    float max_trace_dist;      /* 1e6 cm    ARTS.cpp:284 */
    float surface_offset;      /* 0.1 cm    ARTS.cpp:345 */
    float connect_pullback;    /* 0.1 cm    ARTS.cpp:253 */
    float dist_divisor;        /* 1000      ARTS.cpp:373 */
    float min_seg;             /* 1.0       ARTS.cpp:375 */
    float prob_exponent;       /* 0.1       ARTS.cpp:398 */
    float energy_clamp;        /* 1.0       ARTS.cpp:410 */
    float energy_gain;         /* 10        ARTS.cpp:413 */
    float sound_speed;         /* 343       ARTS.cpp:362 */
    float air_absorption[FS_MAX_BANDS]; /* 0.05 per band, ARTS.cpp:395 */
    int32_t samples_per_bin;   /* 0 = reference's ceil(0.001f*48000) = 49 (FSAC.cpp:324) */
    /* SURVEY A.6-h, HEAD literally: the traces of GeneratePath and ConnectSubpaths query ECC_Pawn as well (ARTS.cpp:243-246,
     * 331-334).  A walk ignores the actor it starts from (AddIgnoredActor, :322-327) but can hit the OTHER end point's
     * collision — and then goes on from there with no material; ConnectSubpaths ignores nothing (:252-254): a connection
     * that starts or ends inside a collision sphere (every connection to B_0 or from F_0) is blocked.  Build-owned engine
     * semantics: an end point's collision is a sphere around its position (ADefaultPawn: 34 cm), a ray that starts
     * inside leaves through the far side.  0 (default) = the end point is a point, nothing collides with it. */
    float listener_radius;     /* cm, 0 = off */
    float source_radius;       /* cm, 0 = off */
} fs_params;

typedef struct fs_stats {
    uint64_t frames;             /* compute_energy_response calls */
    uint64_t rays;               /* subpaths traced by this rank */
    uint64_t pairs;              /* pairs traced by this rank */
    double walk_kernel_ms_sum;    /* HIP-event time on the context's stream, profiling enabled: walk_kernel */
    double walk_kernel_ms_last;
    double connect_kernel_ms_sum; /* connect_kernel */
    double reconstruct_ms_sum;    /* reconstruct_kernel + IR publish copy */
    uint64_t timed_frames;        /* frames contributing to the walk sum */
    uint64_t timed_connects;      /* frames contributing to the connect sum (profiling level 2) */
    uint64_t timed_reconstructs;  /* reconstructs contributing to reconstruct_ms_sum */
    uint32_t bvh_nodes;
    uint32_t triangles;
    uint32_t bvh_stack_need;     /* worst-case traversal stack entries of the committed tree */
    uint32_t bvh_depth;          /* depth of the binary tree before the 4-wide collapse */
    uint64_t scene_bytes;        /* device bytes of BVH + triangles + materials */
    /* work counters kept on the device since the last fs_reset_stats */
    uint64_t segments;           /* walk segments = closest-hit queries the walks TOOK: every walker counts its applied hits and misses and
                                  * leaves the count with its end state; the connect pass, which reads both of a pair's, sums them (a sum
                                  * inside the walk kernel cost the fused launch 20 spilled registers and 3 % of the headline) */
    uint64_t connections_tested; /* any-hit queries: one per pair, or one per (i, j) in all-connections mode */
    uint64_t deposits;           /* unobstructed connections = paths evaluated and deposited */
    /* profiling level 3 only (counting instantiations of the kernels, not for timed frames): records the traversal
     * fetched — 64-B nodes of the 4-wide tree and 48-B triangle records — by the closest-hit queries of the walk and
     * by the any-hit queries of the connections: the kernel's OWN algorithmic bytes (SURVEY.md 8d prices the oracle's
     * BVH2 instead) */
    uint64_t walk_node_fetches, walk_tri_fetches, any_node_fetches, any_tri_fetches;
    uint64_t node_request_insts, node_request_lanes, node_request_distinct;   /* profiling level 3, the dense walk: node-record request
                                  * instructions of its waves, the lanes that took part in them, the distinct 64-B records among those
                                  * lanes — how coherent the requests are (lanes / insts of 64; distinct / lanes: 1 = no two lanes share) */
    uint64_t planned_segments;   /* walk segments as the plan pass predicts them from the RNG stream alone (the roulette does not
                                  * depend on geometry); `segments`, `connections_tested` and `deposits` are what the walk and the
                                  * connect kernels counted as they worked: both must agree (the tests assert it) */
} fs_stats;

/* ---- lifecycle: UAudioRayTracingSubsystem::Initialize/Deinitialize (ARTS.cpp:32-42) ------------- */
void fs_config_default(fs_config* cfg);
void fs_params_default(fs_params* p);
int fs_abi_version(void);
int fs_context_create(const fs_config* cfg, fs_context** out);
int fs_context_destroy(fs_context* ctx);
const char* fs_last_error(const fs_context* ctx); /* replaces UE_LOG warnings; "" if none */
/* Advice of fs_context_create to the host, "" if none — never an error.  Today: GPU_MAX_HW_QUEUES.  The context overlaps
 * the tail of a frame (all-reduce, reconstruct, publish) with the next frame's tracing on two HIP streams; the HIP
 * runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), read once when the runtime initialises.  With
 * other streams in the process the two can share a queue and serialise: export GPU_MAX_HW_QUEUES=16 before the
 * process touches HIP.  The library does not set it for the host. */
const char* fs_context_advice(const fs_context* ctx);

/* ---- scene: RegisterGeometry/UnregisterGeometry (ARTS.h:99-100) + UAcousticMaterial (MAT.h:22-33) -- */
/* xyz: [T][3][3] vertices, mat_id: [T] index into the material table or FS_NO_MATERIAL. Caller keeps ownership. */
int fs_scene_set_triangles(fs_context* ctx, const float* xyz, const uint16_t* mat_id, int32_t T);
/* absorption/transmission/scattering: [M][B] (FAcousticBand arrays, MAT.h:22-30); transmission and
 * scattering may be NULL (the BDPT path reads Absorption only, ARTS.cpp:385). */
int fs_scene_set_materials(fs_context* ctx, const float* absorption, const float* transmission,
                           const float* scattering, int32_t M, int32_t B);
int fs_scene_commit(fs_context* ctx); /* builds the flattened BVH (binned SAH, on the host: 18 ms per 100 000 triangles) and uploads it */
/* The same commit with the tree built ON THE DEVICE (Morton codes, radix sort, Karras' binary radix tree, 4-wide
 * collapse, then the refit pass): well under a millisecond for 100 000 triangles, for actors that register or unregister
 * at run time (RegisterGeometry / UnregisterGeometry, ARTS.h:99-100) in a frame that cannot wait.  Results are identical
 * (closest hits do not depend on the tree); a Morton tree costs more node visits per ray than the SAH tree, so call
 * fs_scene_commit again when there is time.  Falls back to fs_scene_commit by itself for empty scenes, sharded contexts
 * with a communicator (rank 0's build is broadcast) and degenerate inputs. */
int fs_scene_commit_fast(fs_context* ctx);
/* Both: the device-built tree NOW (frames trace through it right away) and the host's SAH tree as soon as a background
 * thread has built it from a snapshot of the registered triangles (18 ms per 100 000 triangles) — the next call that
 * traces anything after that swaps it in (held frames finish first, the stream drains, 8 MB of records are uploaded:
 * ~1 ms once).  Results never change, only the tracing speed (the SAH tree traces 1.6x faster).  Triangles moved by
 * fs_scene_update_triangles in the meantime keep their current positions (re-applied + refit after the swap); a new
 * fs_scene_set_triangles / commit abandons the background build.  fs_scene_refine_pending: is a build still outstanding;
 * fs_scene_refine_wait: block until it has finished and swap now.  fs_context_destroy waits for an outstanding build. */
int fs_scene_commit_progressive(fs_context* ctx);
int fs_scene_refine_pending(fs_context* ctx, int32_t* pending);
int fs_scene_refine_wait(fs_context* ctx);
/* Moving geometry without a rebuild (row f4).  The reference's line traces run against the live physics scene and
 * include ECC_WorldDynamic objects (ARTS.cpp:333-336, FSAC.cpp:229-232): a prop that moved is seen by the next
 * frame.  fs_scene_update_triangles overwrites `count` committed triangles starting at input index `first` with new
 * vertex positions (layout of fs_scene_set_triangles; materials and actor ids are kept); fs_scene_refit recomputes
 * the boxes of the acceleration structure bottom-up on the device (same topology).  A pending refit is also run
 * automatically by the next trace.  Results equal those of a fresh fs_scene_commit of the moved geometry. */
int fs_scene_update_triangles(fs_context* ctx, int32_t first, int32_t count, const float* xyz /* [count][3][3] */);
int fs_scene_refit(fs_context* ctx);
/* Moving actors by transform (row f4).  m[i] is a row-major 3 x 4 affine matrix {r00 r01 r02 tx, r10 r11 r12 ty,
 * r20 r21 r22 tz}: "actor object_ids[i] is now at this transform" — 48 bytes per actor instead of 36 per triangle, one
 * launch for all movers of a tick, and no wait.
 *   Rest pose.  The rest position of a triangle is the position last given for it by fs_scene_set_triangles or
 * fs_scene_update_triangles (which places its triangles at the given world positions, as ever, and makes those their rest
 * positions).  The call is absolute, not cumulative: every triangle whose id (fs_scene_set_objects) is object_ids[i] is
 * placed at m[i] applied to its REST position, whatever transform the object had before.  Objects not listed stay where
 * they are.
 *   Arithmetic, in fp32, each operation rounded, no fused multiply-add: x' = ((r00 x + r01 y) + r02 z) + tx, likewise y'
 * and z', for each of the three vertices; the record (v0, e1, e2, unit normal) is then derived from the three new vertices
 * exactly as fs_scene_update_triangles derives it.  numpy on float32 arrays computes the same bits.  A mirroring or
 * shearing matrix needs no special case.  The identity gives the rest positions back as numbers (a -0.0f coordinate may
 * come back as +0.0f).
 *   Equivalence.  After the call the committed scene is the scene that fs_scene_update_triangles calls carrying those
 * transformed positions would have left, bit for bit, before the refit (records new, boxes old) and after it (box padding
 * included).  The refit is pending and runs before the next trace; fs_scene_refit runs it now.
 *   Later commits.  fs_scene_commit, fs_scene_commit_fast and fs_scene_commit_progressive without a new
 * fs_scene_set_triangles (and the swap of a progressive commit) build over the CURRENT world positions and keep the rest
 * pose: a later transform still maps the rest pose.  fs_scene_set_triangles defines a new rest pose.
 *   Errors.  FS_ERR_INVALID_ARGUMENT: object_ids or m NULL, count < 1, a matrix entry not finite, an id twice in the call,
 * an id that owns no committed triangle, no object ids registered (fs_scene_set_objects(NULL): "every triangle its own
 * actor" has no ids to name), or a transformed coordinate that could leave fp32 — decided from the matrix and the largest
 * rest coordinate c the scene has held, in double: (|r_i0| + |r_i1| + |r_i2|) c + |t_i| > 3e38 for some row i.
 * FS_ERR_NOT_COMMITTED before a commit.  A refused call changes nothing.
 *   Cost.  The caller's arrays are free when the call returns.  Host work is proportional to count, not to the number of
 * triangles.  In the steady state — a count the context has seen before, at most one call between two traced frames — the
 * call neither allocates nor waits for the device.  The first call after a commit uploads the rest positions and the
 * per-object triangle lists once.  A context that never calls it allocates nothing.
 *   Ordering.  Held frames (fs_set_pipelining) finish first, as for every scene call.  Sharded contexts: every rank makes
 * the same call, as with fs_scene_update_triangles.
 *   Not promised: tracing SPEED after large motion.  A refit keeps the tree's topology, so a door swung by 90 degrees sits
 * in inflated boxes until the next fs_scene_commit_progressive.  Results never depend on it. */
int fs_scene_set_object_transforms(fs_context* ctx, const uint32_t* object_ids, const float* m /* [count][12] */, int32_t count);

/* ---- sources and listener: RegisterSource/UnRegisterSource (ARTS.h:103-104, ARTS.cpp:45-53),
 *      GetActorLocation of the source owner / the player pawn (ARTS.cpp:287) ------------------------- */
int fs_source_create(fs_context* ctx, fs_source* out);
int fs_source_destroy(fs_context* ctx, fs_source src);
int fs_source_set_position(fs_context* ctx, fs_source src, const float xyz[3]);
int fs_listener_set_position(fs_context* ctx, const float xyz[3]);
/* The actor a walk starts from is ignored by that walk's traces (FCollisionQueryParams::AddIgnoredActor, ARTS.cpp:322-327): a
 * source whose own mesh is registered geometry does not trap its walks inside it.  object_id = the actor's id among the
 * ids of fs_scene_set_objects; FS_NO_OBJECT (the default) = the end point belongs to no registered actor.  The walks from
 * the source skip the source's actor, the walks from the listener the listener's; ConnectSubpaths ignores nothing
 * (:252-254).  Takes effect with the next traced frame; such frames are not held by fs_set_pipelining. */
#define FS_NO_OBJECT 0xFFFFFFFFu
int fs_source_set_object(fs_context* ctx, fs_source src, uint32_t object_id);
int fs_listener_set_object(fs_context* ctx, uint32_t object_id);

/* ---- source directivity (EXTENDED): every path is weighted by the direction it left the source in ---------------------
 * A source has an orientation f (default (1, 0, 0), UE's forward axis; any finite non-zero vector, normalised in fp32 as
 * f / sqrtf(dot(f, f))) and an optional axisymmetric table T[b][k] of `samples` = K gains per band, sample k at the angle
 * theta_k = k pi / (K - 1) from f (2 <= K <= FS_MAX_DIRECTIVITY_SAMPLES; bands = the context's band count; every gain
 * finite and >= 0, absolute: not normalised).  No table (the default, and gains == NULL) = omnidirectional: today's
 * kernels and results.
 * The emission direction w_e of a connected path: the unit direction of the sphere sample with which the source's walk
 * first HIT something (the exact ray it traced; until then a missed ray leaves the walk at the source); for a path whose
 * walk never left the source, the connection ray's unit direction (from the double end points under
 * FS_FLAG_DOUBLE_POSITIONS).  All-connections modes: per (i, j) the walk's ray if the prefix F_0..F_i has left the
 * source, else the direction of the connection F_i -> B_j.
 * theta = atan2f(|w_e x f|, w_e . f); x = theta (K - 1) / pi, k = min((int)x, K - 2), t = x - k;
 * D_b = T[b][k] + t (T[b][k+1] - T[b][k]) (a constant table gives that constant exactly).  Every deposit of the path
 * gets the factor last: e = min(E_b, energy_clamp) * energy_gain * norm [* MIS weight] * D_b (before the fixed-point
 * conversion of FS_FLAG_DETERMINISTIC).  Applied after the reference's clamp, the weight leaves EvaluatePath untouched and
 * the result is linear in the table.  Sampling, RNG use and MIS weights do not change (the pattern is part of the
 * contribution, not of the sampling density); the result does not depend on sharding.
 * A frame uses the orientation and table in force at its call (also an _async frame whose fs_synchronize comes after a
 * later set call).  Frames of a source with a table are never held by fs_set_pipelining: held frames drain first and
 * the frame runs on its own, like FS_FLAG_DOUBLE_POSITIONS frames.  A new source handle starts omnidirectional, facing
 * (1, 0, 0).  Bad input: FS_ERR_INVALID_ARGUMENT, a bad handle: FS_ERR_BAD_HANDLE; a refused call changes nothing.
 * Not applied by fs_update_sound or fs_trace_rays. */
#define FS_MAX_DIRECTIVITY_SAMPLES 181   /* 1 degree steps */
int fs_source_set_orientation(fs_context* ctx, fs_source src, const float forward[3]);
int fs_source_set_directivity(fs_context* ctx, fs_source src, const float* gains /* [bands][samples] */, int32_t bands,
                              int32_t samples);

/* ---- order window (EXTENDED): a source's traced frames deposit only the paths of some orders -------------------------
 * The traced histogram holds EVERY connected path of the frame: the direct path, the first reflections, the tail.  A host
 * that renders the direct sound (fs_update_direct_paths) and discrete early reflections (fs_update_*_paths) by their own
 * renderers and the traced response as the late field would play those paths twice; the window takes them out of the trace.
 * The ORDER of a contribution is the number of its path's nodes that a walk step's HIT made.  End-to-end connection (the
 * default mode) of F_0..F_k and B_m..B_0: the hits among F_1..F_k plus the hits among B_1..B_m.  Contribution (i, j) of
 * FS_FLAG_ALL_CONNECTIONS / FS_FLAG_MIS_BALANCE: the hits among F_1..F_i plus the hits among B_1..B_j.  A step that misses
 * pushes a duplicate node and adds nothing: (1, 0) over a missed first step is of order 0, like (0, 0) —
 * the order is NOT the step count.  A step that hits an end point's collision sphere (listener_radius, source_radius) is a
 * hit; so is a step of any lobe under FS_FLAG_MATERIAL_LOBES, if it hit.
 * A contribution whose order lies outside [min_order, max_order] (both included) deposits nothing.  Nothing else changes:
 * the walks, the RNG use, the plan pass, the visibility query of every pair or (i, j) and the weights are those of the frame
 * without a window — the uniform weight 1 / N(i + j) and the balance heuristic still count all strategies: the window
 * selects paths, it does not re-normalise.  fs_stats.segments, planned_segments and connections_tested are as without a
 * window; fs_stats.deposits counts what was deposited.  The window depends only on the pair's own walks: not on batching,
 * on the route, or on how pairs are sharded over ranks.  With every flag the window filters what the frame would deposit:
 * FS_FLAG_DETERMINISTIC sums the kept deposits in fixed point, FS_FLAG_ACCUMULATE_ENERGY adds them to the buffer,
 * FS_FLAG_DOUBLE_POSITIONS and FS_FLAG_COSINE_SAMPLING change the walk and not the count; a directivity table weights what
 * is kept.  Reconstruct, FS_FLAG_ROOM_PARAMETERS, the reverb and the text export read the histogram they are given:
 * fs_get_room_parameters of a source with min_order >= 1 describes the response without the direct spike.
 * Default (0, FS_ORDER_UNBOUNDED) = off: today's kernels and results, frames held by fs_set_pipelining as before.  Frames
 * of a source with any other window are never held (held frames drain first; the frame runs on its own, like a directional
 * source's) and may share a batch with plain and directional sources, whose results do not change.  A frame uses the
 * window in force at its call (also an _async frame whose fs_synchronize comes after a later set call).  A new source
 * handle starts at the default.
 * Errors: FS_ERR_BAD_HANDLE for a bad handle; FS_ERR_INVALID_ARGUMENT for min_order < 0, max_order < min_order or a NULL
 * out pointer; a refused call changes nothing.  Which window goes with which renderers: INTEGRATION.md.
 * Not applied by fs_update_sound, fs_trace_rays or the fs_update_*_paths queries. */
#define FS_ORDER_UNBOUNDED 0x7fffffff
int fs_source_set_order_window(fs_context* ctx, fs_source src, int32_t min_order, int32_t max_order);
int fs_source_get_order_window(fs_context* ctx, fs_source src, int32_t* min_order, int32_t* max_order);

/* ---- the hot path ------------------------------------------------------------------------------- */
/* ComputeEnergyResponse() == UpdateSource up to the deposit (ARTS.cpp:128-173): GenerateFullPaths
 * (:201-233) -> GeneratePath x2 (:279-355) -> ConnectSubpaths (:235-277) -> EvaluatePath (:360-420)
 * -> FlushEnergyBuffer + AddEnergyAtDelay(delay, gain/P) (:157-173, FSAC.h:76-91).
 * Traces this rank's share of params->num_rays, leaves the band-major energy [B][num_bins] resident
 * on the device and, if energy_out != NULL, copies it to the host (synchronous). */
int fs_compute_energy_response(fs_context* ctx, fs_source src, const fs_params* params, float* energy_out);
/* Same, enqueue only (no host sync). */
int fs_compute_energy_response_async(fs_context* ctx, fs_source src, const fs_params* params);
/* Several sources in ONE traced frame — UpdateSource over ActiveSources (ForceUpdateSources, ARTS.cpp:60-68, :128-195).
 * Every listed source gets exactly the result of its own fs_compute_energy_response_async(ctx, src, params) call (same
 * pairs, same random streams), but the device runs one plan / walk / connect sequence over all of them: many small
 * frames become one large one (8 sources x 131 072 rays: 1.9x the rays/s of eight separate frames).  Afterwards each
 * source is reconstructed as usual.  The all-connections modes fall back to one frame per source.  A source may appear
 * only once in the list. */
int fs_compute_energy_response_batch_async(fs_context* ctx, const fs_source* sources, int32_t count, const fs_params* params);
/* Device pointer of the energy buffer [B][num_bins] fp32 the source's CURRENT frame deposits into.  A source
 * owns four such buffers and every fs_compute_energy_response* moves on to the next one, so that the tail of
 * frame f (reduce, reconstruct, publish) overlaps the tracing of frame f+1: query the pointer per frame. */
int fs_energy_device_ptr(fs_context* ctx, fs_source src, void** dptr, size_t* bytes);
/* Multi-GPU hook (one sum all-reduce of [B][1000] fp32 between ARTS.cpp:173 and :192).  Hands
 * the current frame's energy buffer over to the context's tail stream: every deposit enqueued so far completes
 * before anything enqueued on *tail_stream after this call.  The caller issues its collective there
 * (ncclAllReduce(dptr, dptr, B*1000, ncclFloat, ncclSum, comm, (hipStream_t)*tail_stream)) and then calls
 * fs_reconstruct_impulse_response_async, which runs behind it on the same stream — all of it concurrent with
 * the next frame's tracing on the compute stream.  Any of the three out-pointers may be NULL.
 * If the frame was computed with FS_FLAG_DETERMINISTIC, *dptr is the [B][num_bins] uint64 fixed-point histogram
 * and *bytes = 8 * B * num_bins: reduce it with an integer sum (ncclUint64 / ncclSum); the reconstruct converts it. */
int fs_energy_handoff(fs_context* ctx, fs_source src, void** dptr, size_t* bytes, void** tail_stream);

/* ---- multi-GPU: the collective behind the boundary --------------------------------------------------
 * The reference's loop over the pairs (GenerateFullPaths, ARTS.cpp:215-230) carries no state from one pair to the next,
 * so rank r of W traces pairs [P r / W, P (r+1) / W) of every frame (fs_config.rank / world_size, one process per GPU)
 * and the ranks sum their [B][bins] histograms: ONE all-reduce per source and frame (fp32, or uint64 in deterministic
 * mode), issued by the library on the context's tail stream at the end of fs_compute_energy_response*, so that it and
 * the reconstruct behind it overlap the next frame's tracing.  With a communicator attached fs_scene_commit also lets
 * rank 0 alone build the acceleration structure and broadcasts it (nodes, triangle records, refit tables).
 * RCCL is opened at run time ($FS_RCCL_LIB if set, else a librccl the process has already loaded, else the system's).
 *   rank 0:     fs_comm_unique_id(id, FS_COMM_ID_BYTES)  -> ship the 128 bytes to the other ranks by any means
 *   every rank: fs_comm_init(ctx, id, FS_COMM_ID_BYTES)  (collective: ncclCommInitRank(world_size, id, rank))
 * or hand over a communicator the host already owns (fs_comm_attach; not destroyed with the context).
 * A world_size > 1 context without a communicator refuses to reconstruct (FS_ERR_COMM) unless the caller reduced the
 * frame itself behind fs_energy_handoff. */
#define FS_COMM_ID_BYTES 128
int fs_comm_unique_id(void* id_out, size_t bytes);
int fs_comm_init(fs_context* ctx, const void* unique_id, size_t bytes);
int fs_comm_attach(fs_context* ctx, void* nccl_comm /* ncclComm_t */);
/* Optional, collective over the ranks, after fs_comm_init / fs_comm_attach: sum the 32 KB energy buffer in ONE exchange
 * step instead of ncclAllReduce (a ring of that size is latency-bound on xGMI).  Every rank owns a mailbox with one slot per
 * rank in its HBM, mapped into the other ranks' processes through HIP IPC (the 64-byte handles travel over the
 * communicator); a reduce = every rank writes its histogram into its slot of every mailbox and raises a sequence flag,
 * then sums the slots of its own mailbox in rank order (bit-identical on all ranks, fp32 or the deterministic mode's
 * u64).  Same stream (the tail stream), same place in the frame as the all-reduce.  If any rank cannot map a peer, all
 * ranks keep ncclAllReduce and the call returns FS_ERR_COMM.  A peer that stops sending makes the next fs_synchronize
 * return FS_ERR_COMM after a bounded wait. */
int fs_comm_enable_oneshot(fs_context* ctx);
int fs_comm_detach(fs_context* ctx);   /* destroys a communicator made by fs_comm_init; fs_context_destroy calls it */
/* What the attached communicator says about itself (ncclCommCount / ncclCommUserRank asked of RCCL now, not the configured
 * values) and how the energy buffer is summed: *collective = 0 none (no communicator), 1 ncclAllReduce on the tail stream,
 * 2 the one-shot peer-write exchange (fs_comm_enable_oneshot).  Without a communicator: *ranks = 0, *rank = -1.
 * A measurement that reports these proves by itself how many ranks took part in its collective. */
int fs_comm_info(fs_context* ctx, int32_t* ranks, int32_t* rank, int32_t* collective);
/* cfg5 — independent sources, one per GPU ("optional ncclAllGather of 8 x 32 KB so any rank can serve any
 * source's IR").  Nothing of a frame is sharded or reduced there (fs_config.world_size stays 1); a PEER communicator
 * of the processes that each own a source serves one collective only:
 *   every rank: fs_peers_init(ctx, id, FS_COMM_ID_BYTES, rank, world_size)        (id from fs_comm_unique_id on rank 0)
 *   every rank: fs_gather_energy(ctx, my_source, out, world_size * B * bins)      (collective, in rank order)
 * out[r] is the [B][bins] histogram of the source rank r passed (its current frame, behind the deposit — and behind the
 * all-reduce on a sharded context).  To serve a peer's IR: fs_update_energy_buffer(mirror_source, out + r * B * bins, …)
 * and fs_reconstruct_impulse_response(mirror_source) — the same energy gives the same samples on every rank.
 * fs_gather_energy_async leaves the gathered histograms on the device, in tail-stream order (valid until the next gather). */
int fs_peers_init(fs_context* ctx, const void* unique_id, size_t bytes, int32_t rank, int32_t world_size);
int fs_peers_detach(fs_context* ctx);   /* fs_context_destroy calls it */
int fs_gather_energy(fs_context* ctx, fs_source src, float* out /* host [world_size][B][bins] */, int32_t n);
int fs_gather_energy_async(fs_context* ctx, fs_source src, void** dptr, size_t* bytes);
/* The partition rule itself, host-only (no device needed): pairs [*pair_begin, *pair_begin + *pair_count) of a frame of
 * num_rays subpaths belong to `rank` of `world_size`. */
int fs_shard_range(uint32_t num_rays, int32_t rank, int32_t world_size, uint32_t* pair_begin, uint32_t* pair_count);

/* Pipelined frames (off by default).  A frame is three passes in a row — plan, walk, connect — and each leaves wave
 * slots idle that the others could use: the walk's longest waves end in a thin tail, the connect pass is one thin
 * round, the plan pass is short.  fs_set_pipelining(ctx, depth):
 *   depth 1  fs_compute_energy_response_async HOLDS BACK the connect pass of its frame; the next call launches it
 *            together with its own walk as ONE kernel;
 *   depth 2  the walk is held back as well: call f launches {plan of frame f, walk of frame f-1, connect of frame f-2}
 *            as one kernel (two kernel boundaries per frame disappear too).
 * The frames in one launch share nothing but the scene (rotating sets of subpath state, schedule, frame scratch and
 * energy buffers).  A held frame's fs_reconstruct_impulse_response_async is recorded and runs right behind its connect
 * pass.  Everything that observes, synchronises or changes what a held frame needs (fs_synchronize, the blocking
 * variants, energy / stats / scene / communicator calls, fs_submit) lets the held frames finish on their own kernels
 * first, so results never depend on the setting; only WHEN work reaches the GPU does: a producer that streams frames
 * (many sources, offline rendering, bench.py) gains 12-14 % (36 % on 16 384-ray frames), a producer that issues one
 * frame per game tick should end the tick with fs_submit (or leave pipelining off) or the frame's IR is published one
 * or two ticks later (three on a single GPU: there the reconstruct of a held frame is itself a part of the launch after
 * the one that connects it, instead of a kernel on the tail stream; four with the library's collective: the launch after
 * next, behind the all-reduce).  Batched frames are held like any other (they gain little: a frame of several chip-fulls has no
 * thin tail to fill).  Frames with lobes, all-connections modes, FS_FLAG_ACCUMULATE_ENERGY and profiling level >= 2
 * are never held.
 * depth = 0 frames (the reference's uncapped walks, ARTS.cpp:294) are held at depth 2 as STAGED WALKS: the longest walk
 * of a frame is a chain of log(subpaths) / log(1 / rr) dependent bounces (118 at 262 144 subpaths) while 97 % of the
 * walks end within 32, so such a frame alone leaves the chip idle for most of its duration.  Launch s + 1 of the frame
 * walks only steps [bound[s-1], bound[s]) of the walks still alive (a 32-byte continuation record per walk carries them
 * from launch to launch), next to the other stages of the frames around it: every launch holds one frame's worth of
 * work and no dependent chain longer than a stage; the frame's IR is published stages + 2 calls after its own (9 with
 * the default bounds 8, 18, 30, 46, 64, 96 — 16, 36, 64, 96 for launches of two to four frames, fs_set_frames_per_launch —;
 * fs_set_walk_stages changes them, count 0 = do not hold such frames). */
int fs_set_pipelining(fs_context* ctx, int32_t depth);   /* 0 = off, 1, 2 */
int fs_set_walk_stages(fs_context* ctx, const int32_t* bounds /* ascending, 1..511 */, int32_t count /* 0..7 */);
/* Frames per launch (with pipelining on; default 1): a 262 144-ray frame leaves a tenth of an MI355X idle that a launch of
 * two such frames fills (866 -> 965 M rays/s).  With n > 1 fs_compute_energy_response_async lets a plain pipelinable frame
 * WAIT until n of its kind have come — the same fs_params but for the low 32 bits of the seed, any sources, the same
 * source several times — and traces them as ONE batched frame in which every item keeps its own seed, energy buffer and
 * recorded fs_reconstruct_impulse_response_async: results are exactly those of n single frames.  Everything that observes
 * or synchronises (and a frame of another kind, and fs_submit) sends a partial group off first.  The price is latency:
 * the IR of a frame is published up to n - 1 calls later than with n = 1.  A waiting frame is traced with the source and
 * listener positions of ITS call (a moved listener sends the group off: a batched frame has one listener). */
int fs_set_frames_per_launch(fs_context* ctx, int32_t n /* 1..4 */);
int fs_submit(fs_context* ctx);   /* hand everything requested so far to the GPU; does not wait */

/* ReconstructImpulseResponse (FSAC.cpp:320-380, called at ARTS.cpp:192): energy -> per-band IR
 * [B][num_samples] and the num_channels-channel view (both channels identical, FSAC.cpp:331) built
 * from the band-mean energy; publishes the channel view to the host front buffer. */
int fs_reconstruct_impulse_response(fs_context* ctx, fs_source src, const fs_params* params);
int fs_reconstruct_impulse_response_async(fs_context* ctx, fs_source src, const fs_params* params);
/* The tick's reconstructs in one go (UpdateSources loops over ActiveSources, ARTS.cpp:100-126, each UpdateSource ending in
 * ReconstructImpulseResponse :192): exactly the result of fs_reconstruct_impulse_response_async on every listed source, as
 * ONE launch that also writes the published channel views, and one completion event — per source the single call costs a
 * stream wait, a kernel, a copy and three event records (32 sources: 2.8 ms per tick against 0.9 ms). */
int fs_reconstruct_impulse_response_batch_async(fs_context* ctx, const fs_source* sources, int32_t count, const fs_params* params);
int fs_synchronize(fs_context* ctx);
/* FS_FLAG_SPECTRAL_IR's crossovers: count == num_bands - 1 inner edges in Hz, strictly ascending, in (0, sample_rate / 2), every
 * band at least one FFT bin wide (sample_rate / K Hz); edges_hz == NULL and count == 0 restore the defaults.  Drains the context
 * (as fs_synchronize) and rebuilds the carriers at the next spectral reconstruct. */
int fs_set_band_edges(fs_context* ctx, const float* edges_hz, int32_t count);
/* UpdateSources (ARTS.cpp:100-126) as the game thread runs it: one UpdateSource (:128-195) for every listed source — trace,
 * deposit, reconstruct — and every IR is in its published host buffer when the call returns.  = the batched compute call +
 * the batched reconstruct + fs_synchronize, with the reconstructs riding on the compute stream (nothing else to overlap
 * with when the caller waits); a depth = 0 frame whose records overflowed is traced again like fs_compute_energy_response
 * — the impulse responses (and sequence numbers) such a failed attempt published meanwhile are PROVISIONAL: the retry publishes
 * the complete ones behind them before the call returns (a concurrent reader may see one for a few hundred microseconds).  So are
 * the FS_FLAG_ROOM_PARAMETERS records published with them (fs_get_room_parameters). */
int fs_update_sources(fs_context* ctx, const fs_source* sources, int32_t count, const fs_params* params);

/* GetImpulseResponse() (FSAC.h:113): pointer to the PUBLISHED [num_samples] channel buffer — a slot of the source's ring of 8
 * pinned host buffers — valid for the next 7 publishes of the source; lock-free and without a runtime call, for the audio
 * thread (RVB.cpp:136).  The buffer is written by the launch that reconstructs the frame (ReconstructImpulseResponse leaves the IR
 * in the component's own buffer, FSAC.cpp:377-378) and becomes the front when fs_get_impulse_response_sequence (or any producer
 * call) has noticed the launch's announcement. */
int fs_get_impulse_response(fs_context* ctx, fs_source src, int32_t channel, const float** data, int32_t* n);
int fs_copy_impulse_response(fs_context* ctx, fs_source src, int32_t channel, float* out, int32_t n);
/* Number of IRs of this source published so far (0: the zero-initialised buffer of FSAC.cpp:24-28 is in front): the k-th
 * reconstruct / fs_set_impulse_response of a source is publish k, and fs_get_impulse_response returns publish
 * `*completed` or a newer one.  Any thread, no lock; it also notices publishes that completed since the producer's last
 * call into the library (a load of the context's publish word; an event query only for the few publishes that went through the
 * tail stream), which fs_get_impulse_response alone does not.  A consumer that reads it before and after
 * copying the buffer knows that the copy is whole (the pointer stays valid for 7 publishes), and the reverb callback can
 * keep the IR's spectrum while the number stands still instead of transforming the IR every callback (RVB.cpp:188). */
int fs_get_impulse_response_sequence(fs_context* ctx, fs_source src, uint64_t* completed);
/* FS_FLAG_ROOM_PARAMETERS: per band b, from the histogram E[k] the reconstruct read (fs_get_energy_buffer of that frame; N =
 * fs_num_bins, dt = (double) bin_duration), in double, each field rounded to float once ("Room parameters"):
 *   energy = sum_k E[k].  A band with a negative or non-finite bin, or no bin > 0, has every other field NaN.
 *   onset  = k0 dt, k0 = the first k with E[k] >= max E / 100 (20 dB below the peak); t_k = (k - k0) dt for k >= k0.
 *   edt, t20, t30: -60 / m, m = the least-squares slope (dB/s) of L[k] = 10 log10(S[k] / S[k0]), S[k] = sum_{j >= k} E[j], over the
 *            k >= k0 with L[k] in [-10, 0], [-25, -5], [-35, -5] dB; NaN with fewer than 2 such points, when no L[k] falls below
 *            the range (the histogram ends first) or when m >= 0.
 *   c50, c80 = 10 log10(early / late) dB, early = sum of E[k >= k0] with t_k < 50 (80) ms, late = the rest from k0 on; +inf when
 *            late is 0.  d50 = early / (early + late) at 50 ms.  ts = sum t_k E[k] / sum E[k] over k >= k0, in seconds.
 * The last bin collects every later arrival and is taken as it is.  An array element: no struct_size. */
typedef struct fs_room_parameters { float energy, onset, edt, t20, t30, c50, c80, d50, ts; } fs_room_parameters;   /* 36 bytes */
/* The records of the FRONT publish (the one fs_get_impulse_response_sequence reports), n == num_bands of them: copied into out and
 * *sequence = that publish's number.  A front publish without records (an unflagged reconstruct, fs_set_impulse_response, none
 * yet) gives *sequence = 0 and leaves out untouched.  Any thread, no lock, no runtime call beyond what
 * fs_get_impulse_response_sequence makes; the copy is whole (it is made again if the front moved by 7 or more meanwhile). */
int fs_get_room_parameters(fs_context* ctx, fs_source src, fs_room_parameters* out, int32_t n, uint64_t* sequence);
int fs_copy_band_impulse_response(fs_context* ctx, fs_source src, int32_t band, float* out, int32_t n);
/* GetImpulseResponse() returns a MUTABLE reference in the reference (FSAC.h:113): consumers may install an IR of their
 * own (the authors' convolver checks used synthetic and downloaded IRs: GenerateDummyImpulseResponse FSAC.cpp:408-452,
 * a delta at samples 0 and N-1; LoadFloatArray :454-490).  Replaces the source's published IR (all channels and
 * bands) with ir[num_samples]; the reverb callback and fs_get_impulse_response see it until the next reconstruct. */
int fs_set_impulse_response(fs_context* ctx, fs_source src, const float* ir, int32_t n);

/* ---- energy-buffer helpers of the component (FSAC.h:72-91), so a UE shim or a test can drive the
 *      same sequence as ARTS.cpp:157-192 ------------------------------------------------------------ */
int fs_get_energy_buffer(fs_context* ctx, fs_source src, float* out, int32_t n);          /* EnergyBuffer */
int fs_flush_energy_buffer(fs_context* ctx, fs_source src);                                /* FSAC.h:76-79 */
int fs_add_energy_at_delay(fs_context* ctx, fs_source src, int32_t band, float delay_seconds,
                           float energy);                                                  /* FSAC.h:87-91 */
int fs_update_energy_buffer(fs_context* ctx, fs_source src, const float* values, int32_t n); /* FSAC.h:81-85 */
int fs_num_bins(const fs_context* ctx);    /* FSAC.h:137 */
int fs_num_samples(const fs_context* ctx); /* FSAC.h:138 */

/* ---- legacy per-frame forward tracer (row a9): UpdateSound (FSAC.cpp:283-306) = RaycastsPerTick specular
 *      chains CastAudioRay (:132-207), each bounce firing a listener-directed CastDirectAudioRay (:209-280),
 *      then OcclusionAttenuation (:295-299), the only live output at HEAD (OCC.cpp:43 reads it).
 *      Engine semantics owned by the build: an actor = an object id per triangle; the player pawn = a sphere. */
typedef struct fs_sound_params {
    uint32_t struct_size;        /* = sizeof(fs_sound_params) */
    int32_t raycasts_per_tick;   /* 1500  FSAC.h:39 */
    uint64_t seed;
    int32_t raycast_bounces;     /* 10    FSAC.h:42 */
    float raycast_distance;      /* 5000  FSAC.h:45 */
    float simulated_duration;    /* 1.0   FSAC.h:136 */
    float listener_radius;       /* pawn collision sphere radius, cm */
} fs_sound_params;

typedef struct fs_sound_result {
    float total_energy;          /* TotalEnergy / RaycastsPerTick, FSAC.cpp:294 (computed then dropped at HEAD) */
    float occlusion_attenuation; /* FSAC.cpp:299 */
    float direct_energy_sum;     /* sum of the per-bounce CastDirectAudioRay results (what Accumulate would get) */
    uint32_t rays_reaching_listener;
    uint32_t direct_hits;
    uint64_t traces;             /* line traces issued */
} fs_sound_result;

void fs_sound_params_default(fs_sound_params* p);
/* actor id per triangle [T] (AActor the collision belongs to); NULL = every triangle its own actor.
 * Takes effect at the next fs_scene_commit. */
int fs_scene_set_objects(fs_context* ctx, const uint32_t* object_id, int32_t T);
int fs_update_sound(fs_context* ctx, fs_source src, const fs_sound_params* p, fs_sound_result* out);
/* GetOcclusionAttenuation() FSAC.h:112: value of the last fs_update_sound (1.0 before the first) */
int fs_get_occlusion_attenuation(fs_context* ctx, fs_source src, float* out);

/* ---- direct paths (EXTENDED): the direct sound of every source of a tick, in one launch -----------------------------------
 * What a host needs to render the direct sound itself: the distance, the arrival time on the impulse response's time axis,
 * how much of the source the listener sees, and how much gets through the surfaces in between, per band.  (In the default
 * mode a traced pair is connected end to end, so the impulse response of a closed room holds almost no direct path; and
 * fs_update_sound's occlusion_attenuation is one centre ray of one source that knows no transmission and no bands.)
 * Deterministic — no random numbers — and specified to the bit: the library is built with -ffp-contract=off; below, every
 * fp32 operation is rounded on its own, in the order written, and fmaf is a fused multiply-add.  numpy float32 scalars
 * compute the same bits.
 *   Sample offsets.  u_0 = (0, 0, 0); for k = 1 .. n-1 with j = k - 1, m = n - 1:  z = 1 - (2 j + 1) / m,
 * rho = sqrt(1 - z z), phi = j pi (3 - sqrt(5)), u_k = (rho cos phi, rho sin phi, z) — computed on the host in double and
 * rounded to float once.  fs_direct_sample_offsets returns exactly the table the kernel uses (FS_ERR_INVALID_ARGUMENT for
 * n < 1, n > FS_MAX_DIRECT_SAMPLES or out == NULL).
 *   chain(o, d, len) -> (reached, crossed, T[bands]).  T_b = 1, crossed = 0, rem = len; for q = 0, 1, ...:
 *     1. !(rem > 0): reached.
 *     2. the closest hit of the ray (o, d) within tmax = rem — the answer fs_trace_rays gives, ignoring nothing;
 *     3. no hit: reached.
 *     4. the hit triangle's object id (fs_scene_set_objects) equals the source's fs_source_set_object id or the listener's
 *        fs_listener_set_object id, and that id is not FS_NO_OBJECT: the ray passes — nothing is counted or multiplied;
 *     5. else crossed += 1; crossed > max_surfaces: blocked, T := 0, end; else T_b = T_b * tau_b with tau_b the transmitted
 *        gain of the hit material (the transmission of fs_scene_set_materials clamped to the absorption and to >= 0;
 *        FS_NO_MATERIAL, an id >= num_materials or no transmission array: 0); every T_b == 0: blocked, end.
 *     6. (4 and 5) adv = t + step; o = (fmaf(adv, d.x, o.x), fmaf(adv, d.y, o.y), fmaf(adv, d.z, o.z)); rem = rem - adv;
 *        q + 1 == FS_DIRECT_MAX_QUERIES: blocked, T := 0, end.
 *   Per source at S, listener at L:  dx = L.x - S.x (dy, dz alike); distance = sqrtf((dx dx + dy dy) + dz dz);
 * delay = (distance / dist_divisor) / sound_speed (EvaluatePath's rule: the direct sound lines up with the impulse response).
 * source_radius == 0: only sample 0 exists (n := 1).  Sample k is VALID when k == 0 or chain(S, u_k, r).crossed == 0 (a
 * sample point behind a wall the source stands close to does not count).  p_k = S + r u_k per component, e = L - p_k,
 * len = sqrtf((e.x e.x + e.y e.y) + e.z e.z); len == 0: the sample is free with T = 1; else inv = 1.0f / len, d = e inv,
 * (reached, crossed, T) = chain(p_k, d, len - pullback).  A sample is FREE when it reached with crossed == 0.
 * samples_valid = V; visibility = (float)free / (float)V; transmission[b] = (float)(sum / (double)V), sum = the double sum
 * of (double)T_k[b] over the valid k in ascending k; surfaces = crossed of sample 0.  An empty committed scene gives free
 * lines.  Nothing depends on which builder made the tree.
 *   Errors.  FS_ERR_INVALID_ARGUMENT: ctx, sources or out NULL, count < 1 or > FS_MAX_DIRECT_BATCH, a struct_size other than
 * sizeof(fs_direct_params), a field outside its range or not finite.  FS_ERR_NO_DEVICE, FS_ERR_BAD_HANDLE,
 * FS_ERR_NOT_COMMITTED as elsewhere.  A handle may appear twice: the rows are independent.  A refused call writes nothing.
 *   Ordering and cost.  Like fs_update_sound: a finished progressive build is installed and a pending refit (also one left
 * by fs_scene_set_object_transforms) runs first; then ONE launch on the compute stream, one copy back and one wait, whatever
 * count is.  Held frames are not flushed; no state of the sources changes (energy, impulse response, occlusion scalar).
 * Staging grows at the first call that needs more: a call with a count and samples the context has seen allocates nothing,
 * and the offset table of a given n is uploaded once per context.  Sharded contexts: any rank may call it, no collective. */
#define FS_MAX_DIRECT_BATCH 256
#define FS_MAX_DIRECT_SAMPLES 64 /* one wave */
#define FS_DIRECT_MAX_QUERIES 32 /* closest-hit queries one ray may chain */
typedef struct fs_direct_params {
    uint32_t struct_size;  /* = sizeof(fs_direct_params) */
    int32_t samples;       /* n, 1 .. FS_MAX_DIRECT_SAMPLES; default 16 */
    float source_radius;   /* r in cm, >= 0, finite; default 0: a point source, only the centre ray */
    int32_t max_surfaces;  /* 1 .. 31; default 8: a ray that would cross more is blocked */
    float step;            /* cm a ray advances past a crossed surface, >= 0; default 0.1 (FSAC.cpp:232) */
    float pullback;        /* cm the ray stops short of the listener, >= 0; default 0.1 (ARTS.cpp:253) */
    float dist_divisor;    /* 1000, as fs_params */
    float sound_speed;     /* 343, as fs_params */
} fs_direct_params;

typedef struct fs_direct_path {
    float distance;        /* cm */
    float delay;           /* s, on the impulse response's time axis */
    float visibility;      /* share of the valid samples with a free line */
    uint32_t surfaces;     /* surfaces the centre ray crossed (counted ones) */
    uint32_t samples_valid;
    float transmission[FS_MAX_BANDS]; /* bands beyond num_bands: 0 */
} fs_direct_path;          /* an array element: no struct_size */

void fs_direct_params_default(fs_direct_params* p);
int fs_direct_sample_offsets(int32_t n, float* out /* [n][3] */); /* host only, needs no context */
int fs_update_direct_paths(fs_context* ctx, const fs_source* sources, int32_t count,
                           const fs_direct_params* params /* NULL = defaults */, fs_direct_path* out /* [count] */);

/* ---- reflection paths (EXTENDED): the first-order specular reflections of every source of a tick -------------------------
 * What a host places between the direct sound (fs_update_direct_paths) and the late field (the traced impulse response, fs_reverb_*):
 * per source the discrete early reflections off single triangles — length, arrival time on the impulse response's time axis,
 * reflection point, the direction the listener hears it from, the reflector and its specular gain per band.  (In the traced impulse
 * response such a reflection is a 1 ms energy bin: no arrival time finer than the bin, no direction, no identity from tick to tick.)
 * The reflectors are found by an exhaustive scan of the triangles, not by sampling: no noise, no seed.  Specified to the bit, like
 * direct paths: the library is built with -ffp-contract=off; below, every fp32 operation is rounded on its own, in the order written,
 * fmaf is a fused multiply-add, a dot product or squared length a.b is (a.x b.x + a.y b.y) + a.z b.z, and cross(a, b) has the
 * components (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x): product, product, subtract.  numpy float32 scalars compute the
 * same bits.  Every discrete decision that could be marginal beyond the filter — which triangle a reflection point lies in, whether a
 * leg is blocked — is taken by the closest-hit query fs_trace_rays answers.
 *   Records.  Triangle i (input order, vertices v0 v1 v2 in force) is known by v0, e1 = v1 - v0, e2 = v2 - v0: one fp32 subtraction
 * per component.  That is exactly what the host build, the device build, fs_scene_update_triangles and the transform kernel of
 * fs_scene_set_object_transforms write into a triangle's record (the last from the vertices it has just computed).
 *   Per source at S with fs_source_set_object id so, listener at L with fs_listener_set_object id lo, for every triangle i:
 *   1. Filter (part of the definition).  n = cross(e1, e2); nn = n.n; nn == 0: rejected.  hS = (S - v0).n, hL = (L - v0).n; kept only
 *      if (hS > 0 && hL > 0) || (hS < 0 && hL < 0).  k = (2 hS) / nn; S' = S - k n per component (the mirror image); D = S' - L.
 *      Moeller-Trumbore on the segment L + s D:  p = cross(D, e2); det = e1.p; det == 0: rejected; inv = 1.0f / det; tv = L - v0;
 *      u = (tv.p) inv; q = cross(tv, e1); v = (D.q) inv; s = (e2.q) inv.  Passed iff u >= -m && v >= -m && u + v <= 1 + m && s > 0 &&
 *      s < 1 with m = margin.  A triangle whose object id equals so or lo, that id not FS_NO_OBJECT, is never a candidate.
 *      candidates = the number of triangles that pass.  candidates > max_candidates: flags = FS_REFLECTION_OVERFLOW, found =
 *      returned = 0 and nothing else of the row is computed (the count is exact even where the list is capped).
 *   2. Leg 1, per candidate.  len1 = sqrtf(D.D); d = D (1.0f / len1); o = L; rem = len1; acc = 0.  For q = 0 ..
 *      FS_DIRECT_MAX_QUERIES - 1: the closest hit of (o, d) within tmax = rem (fs_trace_rays' answer, ignoring nothing) at distance t.
 *      No hit: rejected.  The hit triangle belongs to an own actor (its id equals so or lo, not FS_NO_OBJECT): adv = t + step;
 *      o = fmaf(adv, d, o) per component; rem = rem - adv; acc = acc + adv; next query.  The hit triangle is i: t1 = acc + t,
 *      P = fmaf(t, d, o) per component, accepted.  Any other triangle: rejected.  Out of queries: rejected.
 *   3. Leg 2.  e = S - P; len2 = sqrtf(e.e); len2 == 0: rejected.  d2 = e (1.0f / len2); o2 = fmaf(offset, d2, P) per component;
 *      chain(o2, d2, (len2 - offset) - pullback) of "direct paths" with max_surfaces = 0 and this call's step.  The candidate is
 *      CONFIRMED iff the chain reached with crossed == 0.  No transmission is applied on reflection legs: a leg either passes own
 *      actors only, or the reflection does not exist.
 *   4. Row.  length = t1 + len2; delay = (length / dist_divisor) / sound_speed; point = P; direction = d; triangle = i; material = the
 *      triangle's material id; reflectance[b] = the specular gain of that material, the value the specular lobe of
 *      FS_FLAG_MATERIAL_LOBES multiplies in, for b < num_bands and 0 beyond; a triangle with FS_NO_MATERIAL, an id >= num_materials or
 *      a scene without a material table has reflectance 1 in every band (such a surface applies no material factor in the trace
 *      either).  found = the number confirmed.  The confirmed paths are ordered by (length as fp32 ascending, triangle ascending); the
 *      first returned = min(found, max_paths) are written to the source's max_paths entries of `paths`, the entries beyond
 *      `returned` (all of them for an overflowed row) as all-zero bytes.  Nothing depends on which builder made the tree, on the order
 *      in which candidates were collected, or on count.  An empty committed scene gives rows of zeros.
 *   Errors.  FS_ERR_INVALID_ARGUMENT: ctx, sources, rows or paths NULL, count < 1 or > FS_MAX_REFLECTION_BATCH, a struct_size other
 * than sizeof(fs_reflection_params), a field outside its range or not finite.  FS_ERR_NO_DEVICE, FS_ERR_BAD_HANDLE,
 * FS_ERR_NOT_COMMITTED as elsewhere.  A handle may appear twice: the rows are independent.  A refused call writes nothing.
 *   Ordering and cost.  Like fs_update_direct_paths: a finished progressive build is installed and a pending refit (also one left
 * by fs_scene_set_object_transforms) runs first; then the source table's upload, one clear, TWO launches on the compute stream — the
 * scan of all triangles against all rows, the confirmation of the candidates, a wave per row — one copy back and one wait, whatever
 * count is.  Held frames are not flushed; no state of the sources changes (energy, impulse response, occlusion scalar).  Staging of
 * its own (not that of fs_update_direct_paths) grows at the first call that needs more: a call with a count the context has seen
 * allocates nothing.  Sharded contexts: any rank may call it, no collective. */
#define FS_MAX_REFLECTIONS            16
#define FS_MAX_REFLECTION_CANDIDATES 256
#define FS_MAX_REFLECTION_BATCH      256
#define FS_REFLECTION_OVERFLOW        1u   /* fs_reflection_row.flags */
typedef struct fs_reflection_params {
    uint32_t struct_size;     /* = sizeof(fs_reflection_params) */
    int32_t  max_paths;       /* 1 .. FS_MAX_REFLECTIONS, default 8: rows of `paths` per source */
    int32_t  max_candidates;  /* 1 .. FS_MAX_REFLECTION_CANDIDATES, default 256 */
    float    margin;          /* barycentric slack of the filter, >= 0, finite; default 1e-3 */
    float    step;            /* cm a leg advances past a passed own-actor surface, >= 0; default 0.1 */
    float    offset;          /* cm the second leg starts off the reflector, >= 0; default 0.1 */
    float    pullback;        /* cm the second leg stops short of the source, >= 0; default 0.1 */
    float    dist_divisor;    /* 1000, as fs_params */
    float    sound_speed;     /* 343, as fs_params */
} fs_reflection_params;

typedef struct fs_reflection_path {
    float    length;          /* cm, listener -> reflection point -> source */
    float    delay;           /* s, on the impulse response's time axis: (length / dist_divisor) / sound_speed */
    float    point[3];        /* the reflection point P */
    float    direction[3];    /* unit, from the listener towards P: what a host pans by */
    uint32_t triangle;        /* input index of the reflector */
    uint32_t material;        /* its material id (FS_NO_MATERIAL possible) */
    float    reflectance[FS_MAX_BANDS]; /* bands beyond num_bands: 0 */
} fs_reflection_path;         /* an array element: no struct_size; 72 bytes */

typedef struct fs_reflection_row { uint32_t candidates, found, returned, flags; } fs_reflection_row;

void fs_reflection_params_default(fs_reflection_params* p);
int fs_update_reflection_paths(fs_context* ctx, const fs_source* sources, int32_t count,
                               const fs_reflection_params* params /* NULL = defaults */,
                               fs_reflection_row* rows /* [count] */, fs_reflection_path* paths /* [count][max_paths] */);

/* ---- diffraction paths (EXTENDED): the first-order edge diffraction of every source of a tick -----------------------------
 * What is left of a source that has walked behind a corner or a partition: the sound that bends round ONE free edge of the
 * obstacle — listener -> apex E0 on a triangle edge -> source — late by the detour, from the direction of the edge, the high bands
 * rolled off.  Found like the reflections, by an exhaustive scan of every (triangle, edge): no sampling, no seed, and no edge
 * adjacency — a triangle's record (v0, e1, e2, input index, material, object id) is all the scan reads.  Specified to the bit with
 * the conventions of "reflection paths" (-ffp-contract=off, every fp32 operation rounded on its own in the order written, fmaf
 * fused, a.b = (a.x b.x + a.y b.y) + a.z b.z, cross = product, product, subtract; divide and sqrtf correctly rounded).  Every
 * marginal decision beyond the filter is taken by the closest-hit query fs_trace_rays answers.
 *   Per source at S (actor id so), listener at L (actor id lo), triangle i, edge j = 0, 1, 2 with start a and vector w:
 *   j = 0: a = v0, w = e1;  j = 1: a = v0 + e1, w = e2 - e1;  j = 2: a = v0 + e2, w = -e2 (per component).
 *   1. Filter (part of the definition).  A triangle whose object id equals so or lo, that id not FS_NO_OBJECT, is never a
 *      candidate.  n = cross(e1, e2); nn = n.n; nn == 0: rejected.  hS = (S - v0).n, hL = (L - v0).n; kept only if
 *      (hS > 0 && hL < 0) || (hS < 0 && hL > 0): strictly on opposite sides.  ww = w.w; o = cross(w, n) (in the plane, away from
 *      the triangle's interior); oo = o.o; ww == 0 or oo == 0: rejected.  rS = S - a, rL = L - a; tS = (rS.w) / ww, tL = (rL.w) / ww;
 *      cS = cross(rS, w), cL = cross(rL, w); dS = sqrtf((cS.cS) / ww), dL = sqrtf((cL.cL) / ww); sum = dS + dL; sum == 0:
 *      rejected.  t = tS + ((tL - tS) dS) / sum; kept iff t >= -margin && t <= 1.0f + margin.  E0 = fmaf(t, w, a) per component (not
 *      clamped).  u = S - E0, v = E0 - L; lS = sqrtf(u.u), lL = sqrtf(v.v); lS == 0 or lL == 0: rejected.  length = lS + lL;
 *      g = S - L; distance = sqrtf(g.g); detour = length - distance; kept iff detour <= max_detour.  Shadow zone: s = hS / (hS - hL);
 *      X = fmaf(s, L - S, S) per component (where the segment S -> L meets the plane); kept iff (X - E0).o <= 0 — a lit listener has
 *      no path, and detour -> 0 at the shadow boundary.  candidates = the number of (i, j) that pass.  candidates > max_candidates:
 *      flags = FS_DIFFRACTION_OVERFLOW, confirmed = found = returned = 0 and nothing else of the row is computed.
 *   2. Confirmation, per candidate: three legs, each chain(..) of "direct paths" with max_surfaces = 0 and this call's step (own
 *      actors are passed, anything else blocks).  io = 1.0f / sqrtf(oo), oh = o io; in = 1.0f / sqrtf(nn), nh = n in if hS > 0 else
 *      n (-in): the unit normal towards S.  Eo = fmaf(offset, oh, E0); ES = fmaf(offset, nh, Eo); EL = fmaf(-offset, nh, Eo).
 *      Leg A: e = ES - S, len = sqrtf(e.e); len == 0: reached; else chain(S, e (1.0f / len), len).
 *      Leg B: chain(ES, -nh, 2.0f offset).
 *      Leg C: e = L - EL, len = sqrtf(e.e); len == 0: reached; else chain(EL, e (1.0f / len), len - pullback).
 *      CONFIRMED iff all three reached with crossed == 0 (the verdicts are independent: their order is free).  Leg B rejects the
 *      interior edges of a tessellated wall — Eo lies on the neighbouring triangle — and edges that run into a floor or another
 *      surface; a free rim or a convex corner passes.  confirmed = the number confirmed.
 *   3. Merge.  A convex corner is found once from each face, a vertex shared by two rim edges twice.  key = (length as fp32 bits,
 *      4 i + j), compared as a pair.  A confirmed entry is DROPPED iff some confirmed entry of the row with a smaller key — dropped
 *      itself or not — has q = E0 - E0', q.q < merge merge.  found = the number kept.
 *   4. Row.  The kept entries are ordered by key ascending; the first returned = min(found, max_paths) are written, the entries
 *      beyond `returned` (all of them for an overflowed row) as all-zero bytes.  delay = (length / dist_divisor) / sound_speed;
 *      cos_bend = (u.v) / (lS lL), the cosine between E0 - S and L - E0 (1 = no bend); apex = E0; direction = v (1.0f / lL), from the
 *      listener towards E0; triangle = i, edge = j, material = the triangle's material id;
 *      gain[b] = 1.0f / sqrtf(3.0f + k_b detour) for b < num_bands and 0 beyond: Maekawa's barrier attenuation 10 log10(3 + 20 N)
 *      as an amplitude, with the Fresnel number N = 2 delta f_b / c, i.e. k_b = 40 f_b / (sound_speed dist_divisor), computed by the
 *      host in double and rounded to float once.  f_b = sqrt(lo_b hi_b) of the band's edges in force (fs_set_band_edges, else the
 *      default octave edges); the lowest band's lo is half its hi, the highest band's hi twice its lo (the defaults give 125, 250,
 *      ... Hz), and a single band has f_0 = 1000 Hz.  The gain is an estimate a host is free to ignore: a barrier formula, not
 *      the uniform theory of diffraction, and it contains no distance law.  First order only: a thick obstacle, which needs two
 *      edges, is fs_update_diffraction2_paths' business.  Nothing depends on which builder made the tree, on the order in which candidates were collected, or
 *      on count.  An empty committed scene gives rows of zeros.
 *   The key a host gives the voice of a path (fs_reflection_render_process_batch) is 0x80000000 | (4 triangle + edge): no
 *   reflection's key (its triangle) has the top bit set in a scene of fewer than 2^29 triangles.
 *   Errors, ordering and cost: as fs_update_reflection_paths, with FS_MAX_DIFFRACTION_BATCH — the source table's upload, one clear,
 *   TWO launches (the scan of all triangles against all rows; the confirmation, a wave per row), one copy back and one wait, whatever
 *   count is; staging of its own, grown only at the first call with a larger count.  max_detour must be finite and > 0. */
#define FS_MAX_DIFFRACTIONS            16
#define FS_MAX_DIFFRACTION_CANDIDATES 2048
#define FS_MAX_DIFFRACTION_BATCH      256
#define FS_DIFFRACTION_OVERFLOW        1u   /* fs_diffraction_row.flags */
typedef struct fs_diffraction_params {
    uint32_t struct_size;     /* = sizeof(fs_diffraction_params) */
    int32_t  max_paths;       /* 1 .. FS_MAX_DIFFRACTIONS, default 4: rows of `paths` per source */
    int32_t  max_candidates;  /* 1 .. FS_MAX_DIFFRACTION_CANDIDATES, default 1024 */
    float    margin;          /* slack of the apex's edge parameter, >= 0, finite; default 1e-3 */
    float    max_detour;      /* cm, > 0, finite; default 1000: longer detours are inaudible */
    float    offset;          /* cm the legs' ends stand off the edge, >= 0; default 0.1 */
    float    merge;           /* cm within which two apexes are one path, >= 0; default 1.0 */
    float    step;            /* cm a leg advances past a passed own-actor surface, >= 0; default 0.1 */
    float    pullback;        /* cm the last leg stops short of the listener, >= 0; default 0.1 */
    float    dist_divisor;    /* 1000, as fs_params */
    float    sound_speed;     /* 343, as fs_params */
} fs_diffraction_params;

typedef struct fs_diffraction_path {
    float    length;          /* cm, listener -> apex -> source */
    float    delay;           /* s, on the impulse response's time axis: (length / dist_divisor) / sound_speed */
    float    detour;          /* cm, length - |S - L| */
    float    cos_bend;        /* cosine of the angle the path turns by at the apex; 1 = straight on */
    float    apex[3];         /* E0 */
    float    direction[3];    /* unit, from the listener towards E0: what a host pans by */
    uint32_t triangle;        /* input index of the triangle the edge belongs to */
    uint32_t edge;            /* 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0 */
    uint32_t material;        /* the triangle's material id (FS_NO_MATERIAL possible) */
    float    gain[FS_MAX_BANDS]; /* the barrier estimate; bands beyond num_bands: 0 */
} fs_diffraction_path;        /* an array element: no struct_size; 84 bytes */

typedef struct fs_diffraction_row { uint32_t candidates, confirmed, found, returned, flags; } fs_diffraction_row;

void fs_diffraction_params_default(fs_diffraction_params* p);
int fs_update_diffraction_paths(fs_context* ctx, const fs_source* sources, int32_t count,
                                const fs_diffraction_params* params /* NULL = defaults */,
                                fs_diffraction_row* rows /* [count] */, fs_diffraction_path* paths /* [count][max_paths] */);

/* ---- second-order reflection paths (EXTENDED): the specular reflections off two triangles of every source of a tick -------
 * What fills the gap between the few first-order reflections and the traced late field: listener -> PA on triangle a -> PB on
 * triangle b -> source.  a is the reflector at the listener's end, b the one at the source's end.  Found by an exhaustive scan of the
 * ordered pairs of the triangles near enough to lie on a path within the length cap: no sampling, no seed.  Specified to the bit with
 * the conventions of "reflection paths" (-ffp-contract=off, every fp32 operation rounded on its own in the order written, fmaf
 * fused, a.b = (a.x b.x + a.y b.y) + a.z b.z, cross = product, product, subtract; divide and sqrtf correctly rounded; the records
 * v0, e1, e2; own actors by the ids so / lo).  Every marginal decision beyond the filters is taken by the closest-hit query
 * fs_trace_rays answers.
 *   MT(o, D, k), the Moeller-Trumbore block of the first-order rule's step 1 read for the segment o + s D and triangle k:
 * p = cross(D, e2); det = e1.p; det == 0: rejected; inv = 1.0f / det; tv = o - v0; u = (tv.p) inv; q = cross(tv, e1); v = (D.q) inv;
 * s = (e2.q) inv.  It passes iff u >= -m && v >= -m && u + v <= 1 + m && s > 0 && s < 1 with m = margin.
 *   n_k = cross(e1, e2) and nn_k = n_k.n_k of triangle k.  Per source at S, listener at L:
 *   0. Near set (part of the definition, not an optimisation that may differ).  Triangle k is NEAR iff nn_k != 0, it is not an own
 *      actor's (its object id equals so or lo, that id not FS_NO_OBJECT) and
 *      ((sqrtf(a.a) + sqrtf(b.b)) - (reach + reach)) <= max_length with a = S - v0, b = L - v0 and
 *      reach = fmaxf(sqrtf(e1.e1), sqrtf(e2.e2)): every point of a triangle lies within reach of v0, so a triangle outside this
 *      bound carries no path of at most max_length.  near = their number.  near > max_near: flags = FS_REFLECTION2_NEAR_OVERFLOW,
 *      every other count is 0 and nothing else of the row is computed.
 *   1. Pair filter, for every ordered pair (b, a) of near triangles with a != b.  hS = (S - v0_b).n_b; hS == 0: rejected.
 *      k1 = (2 hS) / nn_b; S1 = S - k1 n_b per component (the image in b).  h1 = (S1 - v0_a).n_a; hL = (L - v0_a).n_a; kept only if
 *      (h1 > 0 && hL > 0) || (h1 < 0 && hL < 0).  k2 = (2 h1) / nn_a; S2 = S1 - k2 n_a (the image of the image); D = S2 - L.
 *      MT(L, D, a) passes and gives s; sqrtf(D.D) <= max_length.  Q = fmaf(s, D, L) per component; hQ = (Q - v0_b).n_b; kept only if
 *      (hQ > 0 && hS > 0) || (hQ < 0 && hS < 0).  D2 = S1 - Q; MT(Q, D2, b) passes.  candidates = the number of ordered pairs that
 *      pass.  candidates > max_candidates: flags = FS_REFLECTION2_OVERFLOW, found = returned = 0 (the count is exact even where
 *      the list is capped).
 *   2. Leg 1, per candidate: the first-order rule's leg 1 from L along D with target a (len1 = sqrtf(D.D); d = D (1.0f / len1);
 *      own actors are passed by adv = t + step; the first other triangle hit must be a).  It yields t1 = acc + t, PA = fmaf(t, d, o)
 *      and the unit direction d.
 *   3. Leg 2.  E = S1 - PA; len2 = sqrtf(E.E); len2 == 0: rejected.  d2 = E (1.0f / len2); o = fmaf(offset, d2, PA) per component;
 *      rem = len2 - offset; acc = 0.  The queries are those of leg 1 (!(rem > 0) before a query or a query without a hit: rejected);
 *      the first triangle hit that is not an own actor's must be b: t2 = offset + (acc + t), PB = fmaf(t, d2, o).  Any other
 *      triangle or running out of queries: rejected.
 *   4. Leg 3, the first-order rule's leg 2 from PB to S.  e = S - PB; len3 = sqrtf(e.e); len3 == 0: rejected.  d3 = e (1.0f / len3);
 *      chain(fmaf(offset, d3, PB), d3, (len3 - offset) - pullback) of "direct paths" with max_surfaces = 0 and this call's step.  The
 *      pair is CONFIRMED iff the chain reached with crossed == 0.
 *   5. Row.  length = (t1 + t2) + len3; delay = (length / dist_divisor) / sound_speed; point[0] = PA, point[1] = PB; direction = d;
 *      triangle[0] = a, triangle[1] = b (input indices); material[0], material[1] their material ids; reflectance[band] =
 *      gA[band] * gB[band], one fp32 multiply of the two specular gains of "reflection paths" (1 for a surface without a material),
 *      0 beyond num_bands.  found = the number confirmed.  The confirmed paths are ordered by (length as fp32 bits, a, b) ascending;
 *      the first returned = min(found, max_paths) are written, the entries beyond `returned` (all of them for an overflowed row) as
 *      all-zero bytes.  Nothing depends on which builder made the tree, on the order of collection or on count.  An empty
 *      committed scene gives rows of zeros.
 *   The key a host gives the voice of such a path (fs_reflection_render_process_batch) is 0x40000000 | (h >> 2) with
 *   h = (a * 2654435761 + b) mod 2^32: disjoint from the first-order keys (a triangle below 2^29) and from the diffraction keys
 *   (0x80000000 | ...).  Two paths of one row may share a key: a host keeps the shorter (the earlier in the row) and drops the other.
 *   Errors, ordering, refusals and staging: as fs_update_reflection_paths, with FS_MAX_REFLECTION2_BATCH — the source table's
 *   upload, one clear (of both counter arrays), THREE launches on the compute stream (the near scan of all triangles against all rows;
 *   the pair filter over every row's near list; the confirmation, a wave per row), one copy back and one wait, whatever count is;
 *   staging of its own, grown only at the first call with a larger count.  max_length must be finite and > 0.
 *   Cost: near^2 pair tests per row.  The default max_length keeps near below the default max_near around a listener in a mine of
 *   100 000 triangles (at most 14 728 of 16 384 for sources within 600 cm; at 2000 cm most such rows overflow). */
#define FS_MAX_REFLECTION2_PATHS         32
#define FS_MAX_REFLECTION2_NEAR       32768
#define FS_MAX_REFLECTION2_CANDIDATES  1024
#define FS_MAX_REFLECTION2_BATCH        256
#define FS_REFLECTION2_OVERFLOW          1u   /* fs_reflection2_row.flags: more candidates than max_candidates */
#define FS_REFLECTION2_NEAR_OVERFLOW     2u   /* fs_reflection2_row.flags: more near triangles than max_near */
typedef struct fs_reflection2_params {
    uint32_t struct_size;     /* = sizeof(fs_reflection2_params) */
    int32_t  max_paths;       /* 1 .. FS_MAX_REFLECTION2_PATHS, default 16: rows of `paths` per source */
    int32_t  max_near;        /* 1 .. FS_MAX_REFLECTION2_NEAR, default 16384 */
    int32_t  max_candidates;  /* 1 .. FS_MAX_REFLECTION2_CANDIDATES, default 256 */
    float    max_length;      /* cm, > 0, finite; default 1500: the longest path looked for */
    float    margin;          /* as fs_reflection_params, default 1e-3 */
    float    step;            /* as fs_reflection_params, default 0.1 */
    float    offset;          /* cm legs 2 and 3 start off their reflector, >= 0; default 0.1 */
    float    pullback;        /* cm leg 3 stops short of the source, >= 0; default 0.1 */
    float    dist_divisor;    /* 1000, as fs_params */
    float    sound_speed;     /* 343, as fs_params */
} fs_reflection2_params;

typedef struct fs_reflection2_path {
    float    length;          /* cm, listener -> PA -> PB -> source */
    float    delay;           /* s, on the impulse response's time axis: (length / dist_divisor) / sound_speed */
    float    point[2][3];     /* PA, PB */
    float    direction[3];    /* unit, from the listener towards PA: what a host pans by */
    uint32_t triangle[2];     /* input indices of a and b */
    uint32_t material[2];     /* their material ids (FS_NO_MATERIAL possible) */
    float    reflectance[FS_MAX_BANDS]; /* gA gB; bands beyond num_bands: 0 */
} fs_reflection2_path;        /* an array element: no struct_size; 92 bytes */

typedef struct fs_reflection2_row { uint32_t near, candidates, found, returned, flags; } fs_reflection2_row;

void fs_reflection2_params_default(fs_reflection2_params* p);
int fs_update_reflection2_paths(fs_context* ctx, const fs_source* sources, int32_t count,
                                const fs_reflection2_params* params /* NULL = defaults */,
                                fs_reflection2_row* rows /* [count] */, fs_reflection2_path* paths /* [count][max_paths] */);

/* ---- second-order diffraction paths (EXTENDED): the diffraction round thick obstacles of every source of a tick -------------
 * What is left of a source behind a wall, a pillar or a crate with thickness: no edge is seen by the source and the listener both,
 * and the shortest sound path bends at TWO edges — source -> apex E1 on the rim of the face towards the source -> apex E0 on the
 * rim of the face towards the listener -> listener.  Index 0 is the listener's end and index 1 the source's, as in
 * fs_reflection2_path.  Found by an exhaustive scan of the ordered pairs of the edge records near enough to lie on a path within the
 * detour cap: no sampling, no seed, no edge adjacency.  Specified to the bit with the conventions of "diffraction paths"
 * (-ffp-contract=off, every fp32 operation rounded on its own in the order written, fmaf fused, a.b = (a.x b.x + a.y b.y) + a.z b.z,
 * cross = product, product, subtract; divide and sqrtf correctly rounded; the records v0, e1, e2; own actors by the ids so / lo).
 * Every marginal decision beyond the filters is taken by the closest-hit query fs_trace_rays answers.
 *   An EDGE RECORD r = (triangle i, edge j) has the start a and the vector w of the first-order rule (j = 0: a = v0, w = e1; j = 1:
 * a = v0 + e1, w = e2 - e1; j = 2: a = v0 + e2, w = -e2), ww = w.w, the triangle's n = cross(e1, e2), nn = n.n and v0,
 * o = cross(w, n), oo = o.o, and the code k_r = 4 i + j (i the input index).  The path is S -> E1 on record q -> E0 on record p -> L.
 * Per source at S, listener at L; g = S - L, distance = sqrtf(g.g):
 *   0. Near set (part of the definition).  Record r is NEAR iff nn != 0, ww != 0, oo != 0, its triangle is not an own actor's, and
 *      ((sqrtf(rS.rS) + sqrtf(rL.rL)) - (reach + reach)) <= distance + max_detour with rS = S - a, rL = L - a, reach = sqrtf(ww):
 *      every point of the edge lies within reach of a, so an edge outside this bound carries no path within the detour cap.
 *      near = their number.  near > max_near: flags = FS_DIFFRACTION2_NEAR_OVERFLOW, every other count is 0 and nothing else of
 *      the row is computed.
 *   1. Pair filter, for every ordered pair (q, p) of near records with q != p; a pair is rejected at the first test it fails.
 *      Parallel: c = w_q.w_p; kept iff c c >= min_parallel (ww_q ww_p).  The two rims of a slab are parallel; skew pairs — over the
 *      top, then round a side — are out of scope.
 *      Gap: r = a_p - a_q; cg = cross(r, w_q); gg = cg.cg; kept iff gg > (merge merge) ww_q — the distance of a_p from q's line
 *      exceeds merge, tested without the divide and the root.  Two records of one geometric edge (a rim found from both its faces)
 *      are the first-order query's business.  g = sqrtf(gg / ww_q).
 *      Apexes, all parameters on q's line: rS = S - a_q, rL = L - a_q; tS = (rS.w_q) / ww_q, tL = (rL.w_q) / ww_q;
 *      cS = cross(rS, w_q), dS = sqrtf((cS.cS) / ww_q); r' = L - a_p, cL = cross(r', w_p), dL = sqrtf((cL.cL) / ww_p);
 *      dt = tL - tS; dSg = dS + g; sum = dSg + dL; sum == 0: rejected.  t1 = tS + (dt dS) / sum; kept iff t1 >= -margin &&
 *      t1 <= 1.0f + margin.  tm = tS + (dt dSg) / sum.  E1 = fmaf(t1, w_q, a_q), P = fmaf(tm, w_q, a_q) per component;
 *      t0 = ((P - a_p).w_p) / ww_p; kept iff t0 >= -margin && t0 <= 1.0f + margin; E0 = fmaf(t0, w_p, a_p).  Nothing is clamped.
 *      This is the closed form of unfolding three half-planes about two parallel lines: for exactly parallel edges the shortest
 *      path, within min_parallel a path whose length is computed from its own points.
 *      Sides: hS = (S - v0_q).n_q, h0 = (E0 - v0_q).n_q; kept iff (hS > 0 && h0 < 0) || (hS < 0 && h0 > 0).  hL = (L - v0_p).n_p,
 *      h1 = (E1 - v0_p).n_p; kept iff strictly opposite likewise.  A slab's rims are found from the faces that look at S and at L;
 *      the face between them is rejected, the other apex lying in its plane.
 *      Shadow zones, the first-order rule's test twice with the other apex as the far end: s1 = hS / (hS - h0);
 *      X1 = fmaf(s1, E0 - S, S); kept iff (X1 - E1).o_q <= 0.  s0 = h1 / (h1 - hL); X0 = fmaf(s0, L - E1, E1); kept iff
 *      (X0 - E0).o_p <= 0.  A pair whose far apex is lit from the near end has no second-order path.
 *      Length: u = S - E1, m = E1 - E0, v = E0 - L; l1 = sqrtf(u.u), lm = sqrtf(m.m), l0 = sqrtf(v.v); any of them 0: rejected.
 *      length = (l1 + lm) + l0; detour = length - distance; kept iff detour <= max_detour.
 *      candidates = the number of pairs that pass (exact even where the list is capped).  candidates > max_candidates:
 *      flags = FS_DIFFRACTION2_OVERFLOW, confirmed = found = returned = 0.
 *   2. Confirmation, per candidate: five legs, each chain(..) of "direct paths" with max_surfaces = 0 and this call's step.  With
 *      the first-order rule's construction at each edge — io = 1.0f / sqrtf(oo), oh = o io; in = 1.0f / sqrtf(nn); nh_q = n_q in if
 *      hS > 0 else n_q (-in), the unit normal of q towards S; nh_p = n_p in if hL > 0 else n_p (-in), that of p towards L:
 *      Eo1 = fmaf(offset, oh_q, E1); ES = fmaf(offset, nh_q, Eo1); EM1 = fmaf(-offset, nh_q, Eo1);
 *      Eo0 = fmaf(offset, oh_p, E0); EL = fmaf(offset, nh_p, Eo0); EM0 = fmaf(-offset, nh_p, Eo0).
 *      Leg 1: e = ES - S, len = sqrtf(e.e); len == 0: reached; else chain(S, e (1.0f / len), len).
 *      Leg 2: chain(ES, -nh_q, 2.0f offset).
 *      Leg 3: e = EM0 - EM1, len likewise; chain(EM1, e (1.0f / len), len): it runs `offset` above the face between the rims.
 *      Leg 4: chain(EM0, nh_p, 2.0f offset); it ends at EL.
 *      Leg 5: e = L - EL, len likewise; chain(EL, e (1.0f / len), len - pullback).
 *      CONFIRMED iff all five reached with crossed == 0 (the verdicts are independent: their order is free).  The short legs 2 and
 *      4 reject the interior edges of tessellated faces and edges that run into another surface, as leg B of the first-order rule.
 *   3. Merge.  key = (length as fp32 bits, k_p, k_q), compared as a triple.  A confirmed entry is DROPPED iff some confirmed entry
 *      of the row with a smaller key — dropped itself or not — has BOTH q0 = E0 - E0', q0.q0 < merge merge and q1 = E1 - E1',
 *      q1.q1 < merge merge.  found = the number kept.
 *   4. Row.  The kept entries are ordered by key ascending; the first returned = min(found, max_paths) are written, the entries
 *      beyond `returned` (all of them for an overflowed row) as all-zero bytes.  delay = (length / dist_divisor) / sound_speed;
 *      gap = g; cos_bend[0] = (m.v) / (lm l0), cos_bend[1] = (u.m) / (l1 lm) (1 = no bend); apex[0] = E0, apex[1] = E1;
 *      direction = v (1.0f / l0), from the listener towards E0; triangle, edge, material [0] of p and [1] of q.
 *      gain[b] = 1.0f / sqrtf(3.0f + (k_b C3) detour) for b < num_bands and 0 beyond, with r = lam5_b / gap; rr = r r;
 *      C3 = (1.0f + rr) / ((1.0f / 3.0f) + rr): ISO 9613-2's double-diffraction term on the first-order barrier formula.  k_b as in
 *      "diffraction paths"; lam5_b = 5 sound_speed dist_divisor / f_b, computed by the host in double and rounded to float once.
 *      C3 goes to 1 as the gap closes — the first-order gain — and to 3 for a wide slab.  Like the first-order gain it is an
 *      estimate a host is free to ignore, and it contains no distance law.  Nothing depends on which builder made the tree, on
 *      the order of collection or on count.  An empty committed scene gives rows of zeros.
 *   The key a host gives the voice of such a path (fs_reflection_render_process_batch) is 0x20000000 | (h >> 3) with
 *   h = (k_p * 2654435761 + k_q) mod 2^32: the one range no other kind uses (first-order reflections below 2^29, second-order
 *   reflections 0x40000000 | ..., first-order diffraction 0x80000000 | ...).  Two paths of one row may share a key: a host keeps the
 *   earlier in the row and drops the other.
 *   Errors, ordering, refusals and staging: as fs_update_diffraction_paths, with FS_MAX_DIFFRACTION2_BATCH — the source table's
 *   upload, one clear (of both counter arrays), THREE launches on the compute stream (the near scan of all edge records against
 *   all rows; the pair filter over every row's near list; the confirmation, a wave per row), one copy back and one wait, whatever
 *   count is; staging of its own, grown only at the first call with a larger count.  max_detour must be finite and > 0,
 *   min_parallel finite, > 0 and <= 1.
 *   Cost: near^2 pair tests per row, near counted in edge records — three per triangle.  The default max_detour keeps near below
 *   the default max_near around a listener in a mine of 100 000 triangles (at most 12 427 of 16 384 for sources within 600 cm; at
 *   500 cm half of such rows overflow, at the first-order call's 1000 cm all of them). */
#define FS_MAX_DIFFRACTION2_PATHS         16
#define FS_MAX_DIFFRACTION2_NEAR       32768
#define FS_MAX_DIFFRACTION2_CANDIDATES  2048
#define FS_MAX_DIFFRACTION2_BATCH        256
#define FS_DIFFRACTION2_OVERFLOW          1u   /* fs_diffraction2_row.flags: more candidates than max_candidates */
#define FS_DIFFRACTION2_NEAR_OVERFLOW     2u   /* fs_diffraction2_row.flags: more near edge records than max_near */
typedef struct fs_diffraction2_params {
    uint32_t struct_size;     /* = sizeof(fs_diffraction2_params) */
    int32_t  max_paths;       /* 1 .. FS_MAX_DIFFRACTION2_PATHS, default 4: rows of `paths` per source */
    int32_t  max_near;        /* 1 .. FS_MAX_DIFFRACTION2_NEAR, default 16384 */
    int32_t  max_candidates;  /* 1 .. FS_MAX_DIFFRACTION2_CANDIDATES, default 1024 */
    float    margin;          /* slack of the apexes' edge parameters, >= 0, finite; default 1e-3 */
    float    max_detour;      /* cm, > 0, finite; default 250: it bounds near, and with it the cost */
    float    min_parallel;    /* squared cosine two edges must reach to count as parallel, in (0, 1]; default 0.999 */
    float    offset;          /* as fs_diffraction_params, default 0.1 */
    float    merge;           /* cm: the least gap, and the distance within which two paths' apexes are one; >= 0; default 1.0 */
    float    step;            /* as fs_diffraction_params, default 0.1 */
    float    pullback;        /* cm leg 5 stops short of the listener, >= 0; default 0.1 */
    float    dist_divisor;    /* 1000, as fs_params */
    float    sound_speed;     /* 343, as fs_params */
} fs_diffraction2_params;

typedef struct fs_diffraction2_path {
    float    length;          /* cm, listener -> E0 -> E1 -> source */
    float    delay;           /* s, on the impulse response's time axis: (length / dist_divisor) / sound_speed */
    float    detour;          /* cm, length - |S - L| */
    float    gap;             /* cm, g: the distance between the two edges' lines, the obstacle's thickness (ISO 9613-2's e) */
    float    cos_bend[2];     /* cosine of the angle the path turns by at E0 and at E1; 1 = straight on */
    float    apex[2][3];      /* E0, E1 */
    float    direction[3];    /* unit, from the listener towards E0: what a host pans by */
    uint32_t triangle[2];     /* input indices of the triangles of p and q */
    uint32_t edge[2];         /* their edges: 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0 */
    uint32_t material[2];     /* their material ids (FS_NO_MATERIAL possible) */
    float    gain[FS_MAX_BANDS]; /* the barrier estimate; bands beyond num_bands: 0 */
} fs_diffraction2_path;       /* an array element: no struct_size; 116 bytes */

typedef struct fs_diffraction2_row { uint32_t near, candidates, confirmed, found, returned, flags; } fs_diffraction2_row;

void fs_diffraction2_params_default(fs_diffraction2_params* p);
int fs_update_diffraction2_paths(fs_context* ctx, const fs_source* sources, int32_t count,
                                 const fs_diffraction2_params* params /* NULL = defaults */,
                                 fs_diffraction2_row* rows /* [count] */, fs_diffraction2_path* paths /* [count][max_paths] */);

/* ---- mixed paths (EXTENDED): one specular reflection and one edge diffraction of every source of a tick ---------------------
 * The last kind of early path of total order two: a path that reflects off one triangle and bends round one edge.  It is what is
 * left of the early reflections of a source that has stepped behind a partition — the reflection off the wall behind it, the floor
 * and the ceiling bounce still reach the listener round the rim, a few dB down and a little later — so that occluded reflections
 * fade rather than vanish.  A path runs listener L -> ... -> source S over one reflector triangle m and one edge record
 * r = (triangle i, edge j) of "second-order diffraction paths"; `end` says where the reflector sits, index 0 the listener's end as
 * everywhere else:
 *   end = 0:  L -> R on m -> E on r -> S          end = 1:  L -> E on r -> R on m -> S
 * A is the end next to the reflector (L for end = 0, S for end = 1), Z the other.  Exhaustive: no sampling, no seed, no edge
 * adjacency.  Specified to the bit with the conventions of "diffraction paths" and "second-order reflection paths"
 * (-ffp-contract=off, every fp32 operation rounded on its own in the order written, fmaf fused, a.b = (a.x b.x + a.y b.y) + a.z b.z,
 * cross = product, product, subtract; divide and sqrtf correctly rounded; the records v0, e1, e2; own actors by the ids so / lo).
 * Every marginal decision beyond the filters is taken by the closest-hit query fs_trace_rays answers.
 *   Per source at S, listener at L:
 *   0. Near set (part of the definition; it bounds the cost).  Triangle k is a near FACE by step 0 of "second-order reflection
 *      paths" with this call's max_length.  Edge record r is a near EDGE iff nn != 0, ww != 0, oo != 0, its triangle is not an own
 *      actor's and ((sqrtf(rS.rS) + sqrtf(rL.rL)) - (reach + reach)) <= max_length with rS = S - a, rL = L - a, reach = sqrtf(ww).
 *      near = the number of near faces plus the number of near edges: one cap covers both.  near > max_near:
 *      flags = FS_MIXED_NEAR_OVERFLOW, every other count is 0 and nothing else of the row is computed.
 *   1. Filter, for every near face m, near edge r = (i, j) and end = 0, 1; a triple is rejected at the first test it fails.
 *      i == m: rejected (compared as triangles: an edge never pairs with its own triangle).
 *      Image: hA = (A - v0_m).n_m; hA == 0: rejected.  k = (2 hA) / nn_m; A' = A - k n_m per component.
 *      Diffraction filter: step 1 of "diffraction paths" for the edge record r, operation by operation, with S := A' for end = 1
 *      and L := A' for end = 0, the other end unchanged (own actors and nn, ww, oo are settled by the near set): hS, hL strictly
 *      opposite, tS, tL, dS, dL, sum != 0, t within margin, E = fmaf(t, w, a), u = S - E, v = E - L, lS, lL != 0, length = lS + lL,
 *      and the shadow-zone test (X - E).o <= 0 with s = hS / (hS - hL), X = fmaf(s, L - S, S).  The rule's `distance` of the
 *      substituted ends, sqrtf(g.g) with g = S - L, is here called unfolded = |A' - Z|; bend_detour = length - unfolded.  Kept
 *      iff bend_detour <= max_detour && length <= max_length.
 *      Reflection point: D = A' - E per component; MT(E, D, m) of "second-order reflection paths" passes with this call's margin.
 *      candidates = the number of (m, r, end) that pass (exact even where the list is capped).  candidates > max_candidates:
 *      flags = FS_MIXED_OVERFLOW, confirmed = found = returned = 0.
 *   2. Confirmation, per candidate: four legs.  hZ = (Z - v0_i).n_i, the rule's hS or hL of the end that is not imaged.  The
 *      first-order rule's construction at the apex with nh the unit normal of the edge's triangle towards Z: io = 1.0f / sqrtf(oo),
 *      oh = o io; in = 1.0f / sqrtf(nn); nh = n in if hZ > 0 else n (-in); Eo = fmaf(offset, oh, E); EZ = fmaf(offset, nh, Eo);
 *      EA = fmaf(-offset, nh, Eo).
 *      Leg 1: e = Z - EZ, len = sqrtf(e.e); chain(EZ, e (1.0f / len), len - pullback) of "direct paths" with max_surfaces = 0 and
 *      this call's step; len == 0: reached.
 *      Leg 2: chain(EZ, -nh, 2.0f offset): the short leg that rejects the interior edges of tessellated surfaces.
 *      Leg 3: D3 = A' - EA; len3 = sqrtf(D3.D3); d = D3 (1.0f / len3); the first-order reflection rule's leg 1 from o = EA along d
 *      with rem = len3: own actors are passed by adv = t + step, the first other triangle hit must be m.  It yields
 *      R = fmaf(t, d, o) per component.  No hit, any other triangle, out of queries: rejected.
 *      Leg 4: e = A - R; len4 = sqrtf(e.e); len4 == 0: rejected.  d4 = e (1.0f / len4);
 *      chain(fmaf(offset, d4, R), d4, (len4 - offset) - pullback) likewise.
 *      CONFIRMED iff legs 1, 2 and 4 reached with crossed == 0 and leg 3 hit m.  confirmed = the number confirmed.
 *   3. Merge.  A convex corner is found once from each of its faces.  key = (length as fp32 bits, end, m, 4 i + j), compared as a
 *      tuple (m, i input indices).  A confirmed entry is DROPPED iff some confirmed entry of the row with a smaller key — dropped
 *      itself or not — has the same end, the same m and q = E - E', q.q < merge merge.  found = the number kept.
 *   4. Row.  The kept entries are ordered by key ascending; the first returned = min(found, max_paths) are written, the entries
 *      beyond `returned` (all of them for an overflowed row) as all-zero bytes.  delay = (length / dist_divisor) / sound_speed;
 *      detour = length - sqrtf(g.g) with g = S - L of the real ends; bend_detour as above; cos_bend = (u.v) / (lS lL) of the filter
 *      (at E in the unfolded space; 1 = no bend); apex = E; point = R; direction = the unit vector from the listener towards the
 *      first point of the path: v (1.0f / lL) for end = 1 (towards E), -d4 per component for end = 0 (towards R); triangle[0] = m,
 *      triangle[1] = i; edge = j; material[0], material[1] their material ids;
 *      gain[b] = gm[b] * (1.0f / sqrtf(3.0f + k_b bend_detour)) for b < num_bands and 0 beyond, gm the reflector's specular gain
 *      of "reflection paths" (1 for a surface without a material), k_b the table of "diffraction paths": the barrier estimate
 *      times the specular gain.  It is an estimate a host is free to ignore — no uniform theory of diffraction — and it contains
 *      no distance law.  Out of scope: more than one reflection with a diffraction, two diffractions with a reflection.
 *      Nothing depends on which builder made the tree, on the order of collection or on count.  An empty committed scene gives
 *      rows of zeros.
 *   The key a host gives the voice of such a path (fs_reflection_render_process_batch) is 0xC0000000 | (h >> 2) with
 *   h = (m * 2654435761 + 4 (2 (4 i + j) + end)) mod 2^32 (the factor 4 keeps the edge and the end above the shift: the two ends of
 *   one reflector and edge record, which a source and a listener either side of a partition both have, get two keys): disjoint from the reflections' keys (below 2^29), the second-order keys
 *   (0x20000000 | ..., 0x40000000 | ...) and, in a scene of fewer than 2^28 triangles, from the first-order diffraction keys
 *   (0x80000000 | (4 triangle + edge) stays below 0xC0000000 there).  Two paths of one row may share a key: a host keeps the
 *   earlier in the row and drops the other.
 *   Errors, ordering, refusals and staging: as fs_update_diffraction2_paths, with FS_MAX_MIXED_BATCH — the source table's upload,
 *   one clear (of both counter arrays), THREE launches on the compute stream (the near scan of all triangles against all rows; the
 *   filter over every row's near list; the confirmation, a wave per row), one copy back and one wait, whatever count is; staging
 *   of its own, grown only at the first call with a larger count.  max_length and max_detour must be finite and > 0.
 *   Cost: (near edges) x (near faces) x 2 filter tests per row, at most near^2 / 2, near counting a triangle up to four times.  The
 *   default max_length keeps near below the default max_near around a listener in a mine of 100 000 triangles (at most 8 472 of
 *   16 384 for sources within 600 cm; at 750 cm 27 of 128 such rows overflow, at 1000 cm 126, at 1500 cm all: measured on the
 *   MI355X, DESIGN.md "Mixed paths").  A room of a few thousand triangles affords 1500 and more. */
#define FS_MAX_MIXED_PATHS         16
#define FS_MAX_MIXED_NEAR       32768
#define FS_MAX_MIXED_CANDIDATES  2048
#define FS_MAX_MIXED_BATCH        256
#define FS_MIXED_OVERFLOW          1u   /* fs_mixed_row.flags: more candidates than max_candidates */
#define FS_MIXED_NEAR_OVERFLOW     2u   /* fs_mixed_row.flags: more near faces and edges than max_near */
typedef struct fs_mixed_params {
    uint32_t struct_size;     /* = sizeof(fs_mixed_params) */
    int32_t  max_paths;       /* 1 .. FS_MAX_MIXED_PATHS, default 8: rows of `paths` per source */
    int32_t  max_near;        /* 1 .. FS_MAX_MIXED_NEAR, default 16384 */
    int32_t  max_candidates;  /* 1 .. FS_MAX_MIXED_CANDIDATES, default 1024 */
    float    max_length;      /* cm, > 0, finite; default 500: the longest path looked for; it bounds near, and with it the cost */
    float    max_detour;      /* cm, > 0, finite; default 1000: the largest bend_detour, as fs_diffraction_params */
    float    margin;          /* slack of the apex's edge parameter and of the reflection point's barycentrics, >= 0; default 1e-3 */
    float    offset;          /* cm the legs' ends stand off the edge and the reflector, >= 0; default 0.1 */
    float    merge;           /* cm within which two apexes are one path, >= 0; default 1.0 */
    float    step;            /* as fs_diffraction_params, default 0.1 */
    float    pullback;        /* cm legs 1 and 4 stop short of their ends, >= 0; default 0.1 */
    float    dist_divisor;    /* 1000, as fs_params */
    float    sound_speed;     /* 343, as fs_params */
} fs_mixed_params;

typedef struct fs_mixed_path {
    float    length;          /* cm, the whole path: |A' - E| + |E - Z| */
    float    delay;           /* s, on the impulse response's time axis: (length / dist_divisor) / sound_speed */
    float    detour;          /* cm, length - |S - L| */
    float    bend_detour;     /* cm, length - |A' - Z|: what the bend alone adds to the reflection's unfolded segment */
    float    cos_bend;        /* cosine of the angle the unfolded path turns by at the apex; 1 = straight on */
    float    apex[3];         /* E */
    float    point[3];        /* R, the reflection point */
    float    direction[3];    /* unit, from the listener towards R (end 0) or E (end 1): what a host pans by */
    uint32_t end;             /* 0: the reflector is next to the listener; 1: next to the source */
    uint32_t triangle[2];     /* input indices of the reflector m and of the triangle i the edge belongs to */
    uint32_t edge;            /* 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0 */
    uint32_t material[2];     /* their material ids (FS_NO_MATERIAL possible) */
    float    gain[FS_MAX_BANDS]; /* specular gain x barrier estimate; bands beyond num_bands: 0 */
} fs_mixed_path;              /* an array element: no struct_size; 112 bytes */

typedef struct fs_mixed_row { uint32_t near, candidates, confirmed, found, returned, flags; } fs_mixed_row;

void fs_mixed_params_default(fs_mixed_params* p);
int fs_update_mixed_paths(fs_context* ctx, const fs_source* sources, int32_t count,
                          const fs_mixed_params* params /* NULL = defaults */,
                          fs_mixed_row* rows /* [count] */, fs_mixed_path* paths /* [count][max_paths] */);

/* ---- pathing (EXTENDED): round several corners by a probe graph ------------------------------------------------------------------
 * A source in the next room but one — down a corridor and through a door, round an S-bend — is answered by none of the six path
 * queries above, and the traced impulse response has no direction.  The host scatters PROBES in free air (a nav-mesh sample, a
 * grid); a BAKE finds which pairs see each other; per tick the shortest route listener -> probes -> source gives a length, the
 * direction the sound arrives from at the listener (which door) and a detour to attenuate by: one more voice per source.
 * Specified to the bit with the conventions of "direct paths": -ffp-contract=off, every fp32 operation rounded on its own in the
 * order written, a.b = (a.x b.x + a.y b.y) + a.z b.z, divide and sqrtf correctly rounded, fmaf fused.  chain(o, d, len) is that
 * section's chain with max_surfaces = 0: it ends `reached` or blocked (at the first triangle that is not an own actor's, or out
 * of queries).  No random numbers; nothing depends on which builder made the tree, on count or on the order of the sources.
 *   Probes.  fs_pathing_set_probes copies count points p_0 .. p_{count-1} (cm, finite; 1 .. FS_MAX_PATHING_PROBES) and drops any
 * bake; count == 0 or xyz == NULL clears the set.  It needs no committed scene.
 *   Bake.  For every pair i < j: e = p_j - p_i per component, w = sqrtf(e.e).  The pair is a CANDIDATE iff
 * w >= FS_PATHING_MIN_EDGE && w <= max_edge.  d = e (1.0f / w) per component.  A candidate is an EDGE iff chain(p_i, d, w) reached,
 * with no own actors (both ids FS_NO_OBJECT) and the bake's step: the ray always runs from the lower index.  The graph is the
 * symmetric bit matrix [N][ceil(N / 32)]: bit (j & 31) of word (j >> 5) of row i says that {i, j} is an edge; the diagonal and the
 * padding bits are zero.  `edges` counts undirected edges.  The bake needs a committed scene (FS_ERR_NOT_COMMITTED) and at least
 * one probe; like fs_update_direct_paths it installs a finished progressive build and runs a pending refit first; it runs on the
 * compute stream (two launches: the upper triangle, a wave per row and block of 64 columns; the mirror), copies the graph back and
 * waits; held frames are not flushed; no collective.  fs_pathing_info: probes, edges (0 before a bake), baked (0 / 1) and
 * scene_changed = 1 iff, since the bake, a commit, fs_scene_update_triangles, fs_scene_refit or fs_scene_set_object_transforms has
 * succeeded (the library installing a progressive build's better tree over unchanged triangles is none of these); 0 before a
 * bake.  It is a report: the library itself never looks at it, the host decides when to bake again.
 *   Update, once per call.  Listener L, its actor id lo.  For every probe k: e = p_k - L, a = sqrtf(e.e); dL[k] = +inf if
 * a > max_attach; 0 if a == 0; else a if chain(L, e (1.0f / a), a) reached with own actor {lo}, +inf if not.
 * d is the fixed point of  d[i] = min(dL[i], min over j adjacent to i of c(j, i)),  c(j, i) = d[j] + w_ji, a c > max_length
 * counting as +inf; w_ji is recomputed as in the bake (it is symmetric: only squares of the components enter).  The fixed point
 * is UNIQUE and reached from d = dL in at most N rounds in any relaxation order (Jacobi, in place, in parallel: the same bits):
 * fp32 addition is monotone in each operand, so each round of any order keeps every d[i] between the fixed point and the value
 * Jacobi has after as many rounds; and with w >= FS_PATHING_MIN_EDGE = 1 and a finite d <= max_length <= FS_PATHING_MAX_LENGTH =
 * 2^20 (half an ulp of d is at most 2^-5), d + w > d strictly, so a route never repeats a probe, has at most N - 1 edges, and
 * Jacobi is done after N rounds.  Two fixed points cannot differ: at the probe where they differ with the smallest value v, v is
 * either dL there (then the other is <= v) or d[j] + w of a neighbour with d[j] < v, on which both agree (then the other is <= v).
 * pred[i] = LISTENER if d[i] == dL[i], else the smallest adjacent j with c(j, i) == d[i].
 *   Update, per source at S with actor id so.  g = S - L per component, distance = sqrtf(g.g).  FS_PATHING_DIRECT is set iff
 * distance == 0 or the centre ray of "direct paths" is free: chain(S, (-g) (1.0f / distance), distance - pullback) reached with own
 * actors {so, lo}.  Probe k with d[k] < +inf QUALIFIES iff e = p_k - S, a = sqrtf(e.e), a <= max_attach and (a == 0 or
 * chain(S, e (1.0f / a), a) reached with own actors {so, lo}); total_k = d[k] + a, kept iff total_k <= max_length.  The path is
 * the smallest total, ties to the smallest k.  None: the row is all-zero bytes except `distance` and the DIRECT bit.  Else
 * flags |= FS_PATHING_FOUND; length = total; delay = (length / dist_divisor) / sound_speed; detour = length - distance;
 * last_probe = k; following pred from k to LISTENER visits `hops` probes, the last of them first_probe (the one next to the
 * listener); with n_0 = first_probe, ..., n_{hops-1} = last_probe, probes[m] = n_m for m < min(hops, FS_MAX_PATHING_NODES) and
 * FS_PATHING_NO_PROBE beyond.  direction = v (1.0f / |v|) with v = P - L, |v| = sqrtf(v.v), P the first point of the sequence
 * (n_0, n_1, ..., S) with |v| != 0; zeros if there is none.  departure likewise from S with v = P - S over (n_{hops-1}, ..., n_0, L).
 * gain[b] = 1.0f / sqrtf(3.0f + k_b detour) with the k_b table of "diffraction paths", 0 beyond num_bands: the barrier estimate of
 * the whole detour, an estimate a host is free to ignore; no distance law.  With validate != 0 each of the hops - 1 baked legs
 * {n_m, n_{m+1}} is run again by the bake's rule with this call's step, from the lower index; a blocked one sets FS_PATHING_STALE
 * and the path is returned all the same (a door has shut since the bake: the host mutes the voice or bakes again).
 *   Out of scope: string-pulling (the route runs through the probes, so length and detour are upper bounds of the taut route's)
 * and more than one path per source.
 *   The key a host gives the voice of such a path is FS_PATHING_VOICE_KEY = 0x80000003: a first-order diffraction key is
 * 0x80000000 | (4 triangle + edge) with edge <= 2, so its low bits are never 11; the mixed keys start at 0xC0000000, the other
 * kinds stay below 0x80000000.  A host renders one voice per FOUND row that is not DIRECT (while the source is in plain sight the
 * direct sound and the early paths speak for it).
 *   Errors.  FS_ERR_INVALID_ARGUMENT: ctx NULL; a count outside its range; a non-finite probe; a struct_size that is not this
 * library's; max_edge, max_attach or max_length not finite and > 0, max_length > FS_PATHING_MAX_LENGTH, step or pullback not finite
 * and >= 0, dist_divisor or sound_speed not finite and > 0; sources or out NULL; a bake without probes; an update or
 * fs_pathing_copy_graph before a bake (also after fs_pathing_set_probes dropped it), or with words != N ceil(N / 32).
 * FS_ERR_NO_DEVICE, FS_ERR_BAD_HANDLE, FS_ERR_NOT_COMMITTED as elsewhere.  A handle may appear twice.  A refused call writes nothing
 * and changes nothing.
 *   Ordering and cost of an update: as fs_update_direct_paths — the source table's upload, THREE launches on the compute stream (the
 * listener's attach chains, a thread per probe; the relaxation, one workgroup with the probes and d in LDS and a hard cap of N
 * rounds, then pred; the sources', one workgroup per row), one copy back and one wait, whatever count is.  The probe set's device arrays are
 * allocated by the first fs_pathing_set_probes for FS_MAX_PATHING_PROBES; staging grows only at the first call with a larger count. */
#define FS_MAX_PATHING_PROBES 1024
#define FS_MAX_PATHING_NODES    16      /* probes of a path that are reported */
#define FS_MAX_PATHING_BATCH   256
#define FS_PATHING_MIN_EDGE   1.0f      /* cm */
#define FS_PATHING_MAX_LENGTH 1048576.0f
#define FS_PATHING_FOUND 1u
#define FS_PATHING_DIRECT 2u
#define FS_PATHING_STALE 4u
#define FS_PATHING_NO_PROBE 0xFFFFFFFFu
#define FS_PATHING_VOICE_KEY 0x80000003u
typedef struct fs_pathing_bake_params {
    uint32_t struct_size;     /* = sizeof(fs_pathing_bake_params) */
    float    max_edge;        /* cm, > 0, finite; default 1000: the longest pair that is tested */
    float    step;            /* as fs_direct_params, default 0.1 */
} fs_pathing_bake_params;

typedef struct fs_pathing_params {
    uint32_t struct_size;     /* = sizeof(fs_pathing_params) */
    int32_t  validate;        /* 0 / 1, default 1: run the path's baked legs again */
    float    max_attach;      /* cm, > 0, finite; default 1000: the farthest probe the listener or a source attaches to */
    float    max_length;      /* cm, > 0, <= FS_PATHING_MAX_LENGTH; default 10000 */
    float    step;            /* as fs_direct_params, default 0.1 */
    float    pullback;        /* cm the DIRECT ray stops short of the listener, >= 0; default 0.1 */
    float    dist_divisor;    /* 1000, as fs_params */
    float    sound_speed;     /* 343, as fs_params */
} fs_pathing_params;

typedef struct fs_pathing_path {
    float    length;          /* cm, listener -> probes -> source */
    float    delay;           /* s, on the impulse response's time axis */
    float    detour;          /* cm, length - distance */
    float    distance;        /* cm, |S - L|: written for every row */
    float    direction[3];    /* unit, from the listener towards the first probe: what a host pans by */
    float    departure[3];    /* unit, from the source towards the last probe */
    uint32_t hops;            /* probes on the path */
    uint32_t flags;           /* FS_PATHING_FOUND | FS_PATHING_DIRECT | FS_PATHING_STALE */
    uint32_t first_probe;     /* the probe next to the listener */
    uint32_t last_probe;      /* the probe next to the source */
    uint32_t probes[FS_MAX_PATHING_NODES]; /* from the listener's end; FS_PATHING_NO_PROBE beyond hops */
    float    gain[FS_MAX_BANDS]; /* barrier estimate of the detour; bands beyond num_bands: 0 */
} fs_pathing_path;            /* an array element: no struct_size; 152 bytes */

int fs_pathing_set_probes(fs_context* ctx, const float* xyz /* [count][3] */, int32_t count /* 0 or xyz NULL: clear */);
void fs_pathing_bake_params_default(fs_pathing_bake_params* p);
int fs_pathing_bake(fs_context* ctx, const fs_pathing_bake_params* params /* NULL = defaults */);
int fs_pathing_info(fs_context* ctx, int32_t* probes, int32_t* edges, int32_t* baked, int32_t* scene_changed); /* any pointer may be NULL */
int fs_pathing_copy_graph(fs_context* ctx, uint32_t* bits /* [N][ceil(N / 32)] */, int32_t words);
void fs_pathing_params_default(fs_pathing_params* p);
int fs_update_pathing_paths(fs_context* ctx, const fs_source* sources, int32_t count,
                            const fs_pathing_params* params /* NULL = defaults */, fs_pathing_path* out /* [count] */);

/* ---- engine line trace the BVH kernel replaces (UWorld::LineTraceSingleByObjectType; call sites
 *      ARTS.cpp:252-254 any-hit, :340-342 closest-hit). Batch query, host arrays. ------------------- */
/* origins/dirs: [N][3] (dirs unit), tmax: [N]; out: hit[N] (0/1), t[N], tri[N] (input triangle index or -1),
 * normal[N][3] (unit, facing the ray origin side). any_hit == 1: only hit[] is written; any_hit == 2 .. 8: the closest
 * hit again, found by the cooperative traversal the small frames' walks use (2, 3, 4: 1, 2, 4 rays per wave — a group of
 * 64, 32, 16 lanes searches each ray — with every node record fetched from memory; 5, 6, 7: the same with the top of the
 * tree resident in LDS; 8: four rays per wave, as much of the tree resident as fits) — same answers, for tests and tools. */
int fs_trace_rays(fs_context* ctx, const float* origins, const float* dirs, const float* tmax, int32_t N,
                  int32_t any_hit, int32_t* hit, float* t, int32_t* tri, float* normal);

/* ---- row f1: the reference's only interchange format (one float per line) --------------------------------
 *      SaveArrayToFile FSAC.cpp:492-505 (FString::SanitizeFloat per value, joined by '\n'),
 *      LoadFloatArray FSAC.cpp:454-490 (split on '\n' culling empty lines, FCString::Atof per line).
 *      Host-side utilities; they need no context and no device. */
int fs_save_array_to_file(const float* data, int32_t n, const char* path);
/* reads at most cap values into out (out may be NULL to count); *n_out = number of lines parsed */
int fs_load_float_array(const char* path, float* out, int32_t cap, int32_t* n_out);
/* "saved_ir.txt": SaveArrayToFile(ImpulseBuffer[channel]) FSAC.cpp:302 */
int fs_save_impulse_response(fs_context* ctx, fs_source src, int32_t channel, const char* path);

/* ---- row f2: the reverb plugin's per-callback convolution (audio render thread) --------------------------
 *      FFrequenSeeAudioReverbPlugin::Initialize/OnInitSource (RVB.cpp:74-109), ProcessSourceAudio (:118-170),
 *      ConvolveFFT (:172-213), FCircularAudioBuffer (CircularBuffer.cpp).  RVB.cpp =
 *      Private/FrequenSeeAudioReverbPlugin.cpp.  The source's most recent impulse response is used on the device. */
#define FS_REVERB_LITERAL_TAIL 1u /* RVB.cpp:147-148 literally: the interleaved buffer's first `frame` floats feed both channels */
int fs_reverb_init(fs_context* ctx, fs_source src, int32_t frame_size /* BufferLength, 1024 */);
/* One source's callback.  in / out: interleaved stereo [frame_size * 2], host; they may be the same buffer.  Per source:
 *  a. apply_reverb == 0 is the bApplyReverb bypass (RVB.cpp:128-132): out := in on the host; neither the device nor any state of
 *     the source (history, write head, crossfade state) is touched.
 *  b. Otherwise out = clamp(IR * u, -1, 1) per channel, u = the source's history followed by this block
 *     (FS_REVERB_LITERAL_TAIL: the block as RVB.cpp:147-148 reads it), with the source's newest device-resident IR — or as
 *     fs_reverb_set_crossfade states, where a fade length is set — and the block enters the history.
 *  c. Audio-thread safe: runs on the context's reverb stream, reads the IR behind the reconstruct that wrote it (events,
 *     exchanged under a per-source mutex held only while work is enqueued) and waits for its own stream only: safe against
 *     the game thread's reconstructs and fs_set_impulse_response.  Not concurrent with fs_reverb_init / _release /
 *     _set_crossfade of the source or another callback: ONE audio render thread runs the callbacks of a context, single and
 *     batched — they share staging owned by the context (rule 5 below), not per-source buffers.
 * fs_reverb_process is fs_reverb_process_batch with one row and no mix; its own checks come first, in this order: a null pointer
 * is FS_ERR_INVALID_ARGUMENT, a bad handle FS_ERR_BAD_HANDLE, a source without fs_reverb_init FS_ERR_INVALID_ARGUMENT. */
int fs_reverb_process(fs_context* ctx, fs_source src, const float* in, float* out, int32_t apply_reverb, uint32_t flags);
/* The callbacks of `count` sources as ONE set of launches (the mixer's loop over ProcessSourceAudio, RVB.cpp:118-170): the
 * number of copies, kernel launches and stream synchronisations of a call does not grow with count.
 *   in  [count][frame_size * 2]  interleaved stereo, host; row i belongs to sources[i]
 *   out [count][frame_size * 2]  or NULL
 *   apply_reverb [count]         or NULL = all on; flags (FS_REVERB_LITERAL_TAIL) hold for every source of the call
 *   mix [frame_size * 2]         or NULL; out == NULL && mix == NULL is FS_ERR_INVALID_ARGUMENT
 *  1. Rules a - c above per row, in list order: out[i] and the state of sources[i] afterwards are those of rule a or b with
 *     (sources[i], in[i], apply_reverb[i], flags), to the bit the same whether the sources are served by one call or by several
 *     (crossfades included).  Batch and single calls may be mixed freely from one callback to the next.
 *  2. mix[j] = ((out[0][j] + out[1][j]) + out[2][j]) + ... in fp32, in list order, over the values of rule 1 (each clamped; a
 *     bypassed source contributes its input); the sum itself is not clamped.  It is computed on the device in that fixed
 *     order (reproducible); with out == NULL only mix comes back from the device.
 *  3. 1 <= count <= FS_MAX_REVERB_BATCH, every source has had fs_reverb_init, all share one frame size, no handle appears
 *     twice: otherwise FS_ERR_INVALID_ARGUMENT (FS_ERR_BAD_HANDLE for a bad handle).  A refused call changes nothing.
 *  4. The threading contract of rule c for every listed source.  The sources' mutexes are taken in the order the game thread
 *     takes them and held only while work is enqueued.
 *  5. Pinned staging owned by the context is grown at the FIRST call that needs more (count x frame_size); a call whose
 *     count and frame size the context has already seen allocates no device or pinned memory. */
#define FS_MAX_REVERB_BATCH 256
int fs_reverb_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in, float* out,
                            const int32_t* apply_reverb, uint32_t flags, float* mix);
int fs_reverb_release(fs_context* ctx, fs_source src); /* OnReleaseSource: ClearBuffers; also ends a running crossfade */
/* Crossfade between successive impulse responses (not in the reference, which switches abruptly; opt-in per source).
 * samples == 0 (the default): every callback convolves with the IR on the device at that moment, the reference's switch.
 * 1 <= samples <= 4 * sample_rate: the fade length L; anything else is FS_ERR_INVALID_ARGUMENT.  May be set before or after
 * fs_reverb_init, under the same threading contract (never concurrently with the source's callback); every call ends a
 * running fade at its target IR.  With L > 0 the callback keeps two IRs of its own on the device, h_from and h_to:
 *  1. It sees the IR the default path would (the newest reconstruct's or fs_set_impulse_response's, waited for through the
 *     same events).  When that IR is newer than h_to, a fade to it starts at this callback's first output sample; of several
 *     rewrites between two callbacks only the newest counts.
 *  2. With p = output samples since the fade began and g = (p + 1) / L while p < L:
 *       y[s] = clamp((1 - g) (h_from * u)[s] + g (h_to * u)[s], -1, 1)
 *     where u is the input the default path convolves (FS_REVERB_LITERAL_TAIL selects it as there).  At p = L the fade is
 *     complete (h_from := h_to) and callbacks convolve one IR again.
 *  3. A new IR p0 samples into a fade: h_from := (1 - p0 / L) h_from + (p0 / L) h_to (the IR heard at the last output sample),
 *     then a fade from there to the new IR.  Exact (the convolution is linear in the IR): never more than two convolutions.
 *  4. The first callback after fs_reverb_init or after enabling takes the current IR without a fade.  fs_reverb_release
 *     clears the history and ends any fade; the bypass (apply_reverb == 0) touches no fade state.
 *  5. The fade is linear, not equal-power: successive IRs of one source are strongly correlated (equal power would raise the
 *     level by up to 3 dB mid-fade). */
int fs_reverb_set_crossfade(fs_context* ctx, fs_source src, int32_t samples);
/* The engine that computes rule b's convolution, per source.  DIRECT (the default of a new source handle) evaluates the sum
 * tap by tap: 2 * frame_size * num_samples MACs per callback and a history ring that bounds the IR (fs_reverb_init).
 * PARTITIONED is a uniformly partitioned overlap-save convolution with a frequency-domain delay line: with F = frame_size,
 * N = the smallest power of two >= 2 F and K = ceil(num_samples / F), the IR is kept as K spectra H_p = FFT_N(h[pF .. pF + F)),
 * every callback transforms one window X_t = FFT_N(w_L + i w_R) of the last N samples into a ring of K spectra, and
 * out = the last F samples of IFFT_N(sum_p H_p X_{t-p}), real part left, imaginary part right: K N complex MACs and three
 * transforms, a history of one window whatever the IR length.
 *  - The call only records the choice: it takes effect at the source's next fs_reverb_init, as the frame size does; until then
 *    the source keeps the engine it was initialised with.  Threading contract of fs_reverb_set_crossfade.
 *  - fs_reverb_init under PARTITIONED accepts 16 <= frame_size <= 2048 and any num_samples <= 1 048 576 (no ring limit), anything
 *    else is FS_ERR_INVALID_ARGUMENT; it allocates all of the engine's per-source device memory (the second spectrum set of a
 *    crossfade: there or in fs_reverb_set_crossfade), so batch rule 5 holds.  Under DIRECT its checks are unchanged.
 *  - Every rule beside fs_reverb_process, fs_reverb_process_batch and fs_reverb_set_crossfade holds for a partitioned source, with
 *    "to the bit" in batch rule 1 read as "to the bit between calls that serve the source with the same engine": a partitioned
 *    source gives the same bits served by one call or several, alone or in any batch; the two engines agree with each other
 *    within rounding (both within 2e-5 of the double-precision convolution, relative to the block's peak).  A batch may mix
 *    sources of both engines at one frame size; its direct rows keep their bits.
 *  - The spectra are built from the device-resident IR only by a callback that sees a newer IR than the one they hold (and by
 *    the first after fs_reverb_init): only such a callback waits for a reconstruct.  Crossfade rule 3's fold is done on the
 *    spectra (exact: the transform is linear); a fading source forms both products and mixes them per output sample.
 *  - FS_REVERB_LITERAL_TAIL: the transform used in the callback is that of the window ending in the block as RVB.cpp:147-148
 *    reads it; the transform of the true samples enters the ring (one more forward transform in such a callback).
 * A null context is FS_ERR_INVALID_ARGUMENT, no device FS_ERR_NO_DEVICE, a bad handle FS_ERR_BAD_HANDLE, an engine other than
 * these two FS_ERR_INVALID_ARGUMENT; a refused call changes nothing. */
#define FS_REVERB_ENGINE_DIRECT      0   /* the tap-by-tap kernels, the default */
#define FS_REVERB_ENGINE_PARTITIONED 1
int fs_reverb_set_engine(fs_context* ctx, fs_source src, int32_t engine);
/* Two-ear late reverb (EXTENDED; DESIGN.md section 8, "Two-ear late reverb").  A reconstruct publishes one channel row, and the
 * callback convolves both input channels with it: the tail of a mono source sits inside the head.  A source with EARS convolves
 * the left input with h_L and the right with h_R, two IRs with the interaural coherence of a diffuse field — the late field has no
 * direction, only the coherence gamma(f) of two points a head's width apart.  Nothing in the trace or the reconstruct changes.
 *
 * The ear carriers are context-wide and use the bands, the bin assignment and K (the smallest power of two >= num_samples) of
 * FS_FLAG_SPECTRAL_IR, fs_set_band_edges included:
 *   1. bin k in [1, K/2), in double: f_k = k fs / K;  x_k = 2 pi f_k (2 radius_cm) / sound_speed_cm_s;
 *      gamma_k = sin(x_k) / x_k (1 at x_k = 0);  a_k = sqrt((1 + gamma_k) / 2),  b_k = sqrt((1 - gamma_k) / 2).
 *   2. mid spectrum of band b: a_k exp(i phi_k) on the band's bins, phi_k = 2 pi (splitmix64(0x5EED + k) >> 40) 2^-24 (the
 *      spectral IR's phase);
 *   3. side spectrum of band b: b_k exp(i psi_k), psi_k = 2 pi (splitmix64(0x5EED0EA2 + k) >> 40) 2^-24;
 *   4. each product of 2 and 3 is formed in double and rounded to float once;
 *   5. r^M_b, r^S_b = the real inverse transforms of those spectra (the spectral IR's inverse passes);
 *   6. one scale per band for both rows: g_b = sqrt(N / sum_{n<N} (r^M_b[n]^2 + r^S_b[n]^2)), the sum in double;
 *      cm_b = g_b r^M_b, cs_b = g_b r^S_b;
 *   7. the left carrier is cm_b + cs_b, the right cm_b - cs_b: mean power (L^2 + R^2) / 2 = 1 over the IR, coherence
 *      a_k^2 - b_k^2 = gamma_k per bin.
 * Per source:
 *   8. m[n] = (1/sqrt(B)) sum_b env_b[n] cm_b[n], s[n] likewise with cs_b; env_b = the source's device-resident band row b
 *      (what fs_copy_band_impulse_response copies), whatever flags the reconstruct had; after fs_set_impulse_response every band
 *      row is the installed IR;
 *   9. the sums are fp32 in ascending band order (the exact expression: DESIGN.md);
 *  10. h_L = m + s, h_R = m - s.
 * The callback of a source with ears gives out_L = clamp(h_L * u_L), out_R = clamp(h_R * u_R), u exactly what the partitioned
 * engine convolves (FS_REVERB_LITERAL_TAIL included); every rule of fs_reverb_process_batch, fs_reverb_set_crossfade and
 * fs_reverb_set_engine holds with "the IR" read as the pair.
 *
 * fs_reverb_ears_set (game thread; desc == NULL: clear) builds the set on the compute stream and waits for it.  Threading
 * contract of fs_reverb_init: never concurrent with a callback.  radius_cm >= 0 (0: gamma = 1, s = 0, the two ears are equal),
 * sound_speed_cm_s > 0, both finite, struct_size as fs_reverb_ears_default fills it; the band edges in force must give every band
 * a bin (FS_FLAG_SPECTRAL_IR's condition and text) — else FS_ERR_INVALID_ARGUMENT and nothing changes.  Replacing a set makes
 * every source initialised with ears take again at its next callback (through its crossfade, if it has one); clearing is
 * FS_ERR_INVALID_ARGUMENT while such a source exists.  fs_set_band_edges with a set installed rebuilds it, under the same contract.
 * fs_reverb_set_ears records the choice like fs_reverb_set_engine: it takes effect at the source's next fs_reverb_init, which is
 * FS_ERR_INVALID_ARGUMENT with ears on when the source's engine is not FS_REVERB_ENGINE_PARTITIONED or no set is installed (the
 * message says which).  That init allocates the second spectrum set ([2][K][N] per IR copy): the callback allocates nothing.
 * fs_reverb_copy_ear_impulse_responses (game thread, ordered like fs_copy_band_impulse_response; needs an installed set, not
 * fs_reverb_init) copies h_L and h_R of the source's newest device-resident IR, n = fs_num_samples each — for hosts with a
 * convolver of their own. */
typedef struct fs_reverb_ears_desc {
    uint32_t struct_size;
    float    radius_cm;          /* FS_HRTF_DEFAULT_RADIUS_CM */
    float    sound_speed_cm_s;   /* FS_HRTF_DEFAULT_SOUND_SPEED_CM_S (real physics, as fs_hrtf_spherical_head) */
} fs_reverb_ears_desc;
void fs_reverb_ears_default(fs_reverb_ears_desc* desc);
int fs_reverb_ears_set(fs_context* ctx, const fs_reverb_ears_desc* desc /* NULL: clear */);
int fs_reverb_ears_info(fs_context* ctx, float* radius_cm, float* sound_speed_cm_s, int32_t* installed); /* any pointer may be NULL */
int fs_reverb_set_ears(fs_context* ctx, fs_source src, int32_t on);
int fs_reverb_copy_ear_impulse_responses(fs_context* ctx, fs_source src, float* left, float* right, int32_t n);

/* ---- direct sound on the audio thread (EXTENDED): what fs_update_direct_paths' rows are rendered with ---------------------
 *      The reference's slot is FFrequenSeeAudioOcclusionPlugin::ProcessAudio (Private/FrequenSeeAudioOcclusionPlugin.cpp:33-50),
 *      which fetches the occlusion scalar and leaves the multiply commented out; its DopplerActor fakes the pitch shift with a
 *      SetPitchMultiplier.  Here both are one block per source, for all sources of a callback in one set of launches: a
 *      time-varying fractional delay (which IS the Doppler shift) and a short linear-phase FIR whose taps are
 *      sum_b band_gain[b] * k_b, k_b a fixed band kernel.  No panning, no distance attenuation: those stay the host's.
 *   Band kernels.  T = taps, odd, 1 .. FS_DIRECT_RENDER_MAX_TAPS; c = (T - 1) / 2; m = t - c.
 *     w[m] = 0.5 + 0.5 cos(pi m / (c + 1));  L_f[m] = sin(2 pi f m / fs) / (pi m) for m != 0, L_f[0] = 2 f / fs.
 *     Edges e_0 = 0 (L := 0); e_1 .. e_{B-1} the inner edges — the floats given, or 125 * 2^(b - 0.5) when edges_hz is NULL;
 *     e_B = Nyquist with L := the unit impulse at m = 0, taken exactly, so that the bands telescope to a delta.
 *     k_b[t] = w[m] (L_{e_{b+1}}[m] - L_{e_b}[m]), computed on the host in double and rounded to float once.
 *   fs_direct_band_kernels writes that table [bands][taps]; host only, no context, no device.  FS_ERR_INVALID_ARGUMENT: out
 *   NULL, bands outside 1 .. FS_MAX_BANDS, taps even or out of range, sample_rate < 1, edges that are not finite, not strictly
 *   ascending or not inside (0, sample_rate / 2).  fs_direct_render_init builds exactly this table from the context's sample
 *   rate, band count and the edges in force (fs_set_band_edges, else the defaults) and uploads it once per (context, T, edges).
 *   What the formula gives (measured on the CPU): with unit gains the taps are a delta within 1.3e-8; T = 255 separates the
 *   octave bands from 500 Hz up and blends 125 and 250 Hz, T = 1023 separates all eight; the output is late by c samples —
 *   2.6 ms at the suggested default T = 255 and 48 kHz — which the host may subtract from `delay`.
 *   State per source, all device-resident, all allocated by fs_direct_render_init: a zeroed history ring per channel, an
 *   absolute sample counter n0, the last delay d0 (samples), the last gains g0, a primed flag.  D = ceil(max_delay_seconds fs);
 *   the ring is the smallest power of two >= D + T + 1 + F floats, and D + T + 1 + F <= 2^20; 16 <= F = frame_size <= 16384:
 *   otherwise FS_ERR_INVALID_ARGUMENT (also for even T, and for edges in force that do not lie in (0, fs / 2)).  Calling it again
 *   re-initialises the source with the new F, T and D.  fs_direct_render_release: history := 0, and the next callback takes
 *   its target without a ramp (a source without fs_direct_render_init: nothing to do, FS_OK).
 *   One callback, per row.  fp32 throughout; every operation is rounded on its own, in the order written (the library is built
 *   with -ffp-contract=off); numpy float32 computes the same bits.
 *     Target.  d1 = delay * (float)fs; g1 = band_gain.  A delay that is negative, not finite or with d1 > D, or a gain (of a
 *       band < num_bands) that is negative or not finite, refuses the WHOLE call: nothing changes, nothing is enqueued.
 *     First callback (not primed): d0 := d1, g0 := g1.
 *     Slew limit.  e = clamp(d1 - d0, -F/2, +F/2): a teleport glides at half a sample per sample instead of clicking.  The
 *       state after the call is d0 + e — what the last output sample used — and g1.
 *     Taps.  cA[t] = sum over b ascending of (c = c + gA[b] * k_b[t], from 0), A = 0, 1;  dc[t] = c1[t] - c0[t].
 *     Output s (0 .. F-1) of channel ch, x(n) the channel's sample at absolute index n (zero before the stream began):
 *       a = (float)(s + 1) / (float)F;  d = d0 + a * e;  i = floorf(d), f = d - (float)i;  c = c0[t] + a * dc[t];
 *       p = n0 + s - t - i;  v = x(p) + f * (x(p - 1) - x(p));
 *       four accumulators: acc_j takes the taps t = j (mod 4) in ascending t, acc_j = acc_j + c * v;
 *       y = (acc_0 + acc_1) + (acc_2 + acc_3).  Not clamped (the reference's multiply has no clamp).
 *     The accumulator order is part of the contract: a source gives the same bits served alone or in any batch.
 *     Afterwards the block enters the history and n0 += F.
 *   fs_direct_render_process_batch.
 *     in  [count][frame_size * 2]  interleaved stereo, host; row i belongs to sources[i] and targets[i]
 *     out [count][frame_size * 2]  or NULL
 *     mix [frame_size * 2]         or NULL; out == NULL && mix == NULL is FS_ERR_INVALID_ARGUMENT
 *    1. Per row, in list order, the rule above: out[i] and the state of sources[i] afterwards are, to the bit, the same whether
 *       the sources are served by one call or by several.
 *    2. mix[j] = ((out[0][j] + out[1][j]) + out[2][j]) + ... in fp32, in list order; computed on the device in that fixed
 *       order (reproducible); with out == NULL only mix comes back from the device.
 *    3. 1 <= count <= FS_MAX_DIRECT_RENDER_BATCH, every source has had fs_direct_render_init, all share one frame size and one
 *       T, no handle appears twice, every target is legal: otherwise FS_ERR_INVALID_ARGUMENT (FS_ERR_BAD_HANDLE for a bad
 *       handle; a null pointer FS_ERR_INVALID_ARGUMENT, no device FS_ERR_NO_DEVICE).  A refused call changes nothing.
 *    4. Audio-thread safe: runs on the context's reverb stream and waits for that stream only.  It reads no impulse response
 *       and takes no source mutex.  Not concurrent with fs_direct_render_init / _release of a listed source or another
 *       callback (reverb or direct): ONE audio render thread runs the callbacks of a context.
 *    5. Staging of its own, owned by the context (pinned host + device; not the reverb callback's and not
 *       fs_update_direct_paths'), grown at the FIRST call that needs more (count x frame_size); a call whose count and frame
 *       size the context has already seen allocates no device or pinned memory.  One copy up, a number of launches that does
 *       not grow with count, one copy back, one wait.
 *   fs_source_destroy and fs_context_destroy free everything. */
#define FS_MAX_DIRECT_RENDER_BATCH 256
#define FS_DIRECT_RENDER_MAX_TAPS  2047
typedef struct fs_direct_render_target {
    float delay;                   /* s, >= 0: fs_direct_path.delay, less whatever latency the host compensates */
    float band_gain[FS_MAX_BANDS]; /* finite, >= 0; entries beyond num_bands ignored */
} fs_direct_render_target;         /* an array element: no struct_size; 36 bytes */
int fs_direct_band_kernels(int32_t sample_rate, const float* edges_hz /* [bands - 1], or NULL = the default octave edges */,
                           int32_t bands, int32_t taps, float* out /* [bands][taps] */);
int fs_direct_render_init(fs_context* ctx, fs_source src, int32_t frame_size, int32_t taps, float max_delay_seconds);
int fs_direct_render_release(fs_context* ctx, fs_source src);
int fs_direct_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in,
                                   const fs_direct_render_target* targets /* [count] */, float* out, float* mix);

/* ---- early reflections on the audio thread (EXTENDED): what fs_update_reflection_paths' paths are rendered with -----------
 *      Not in the reference.  Per source a VOICE BANK: up to `voices` slots, each one exactly the direct renderer's block above (a
 *      fractional, slew-limited delay — the Doppler shift — and the band FIR) reading ONE history ring shared by all slots of the
 *      source, weighted by a per-channel gain (where the host's pan and distance law go) and summed.  Voices are matched from
 *      callback to callback by a key (the reflector's triangle); a voice whose key appears fades in over one block, one whose key
 *      disappears fades out over one block: a reflection that switches on or off at a block boundary does not click.  All sources
 *      of a callback share one set of launches.  The library applies only the gains it is given.
 *   Band kernels.  The table of fs_direct_band_kernels for the context's sample rate, band count and edges in force: the very
 *   upload fs_direct_render_init uses for the same (context, T, edges).
 *   fs_reflection_render_init.  F = frame_size, T = taps, D = ceil(max_delay_seconds fs) under fs_direct_render_init's limits
 *   (16 <= F <= 16384; T odd, 1 .. FS_DIRECT_RENDER_MAX_TAPS; the ring is the smallest power of two >= D + T + 1 + F floats and
 *   D + T + 1 + F <= 2^20; edges in force inside (0, fs / 2)), and 1 <= V = voices <= FS_MAX_REFLECTION_VOICES: otherwise
 *   FS_ERR_INVALID_ARGUMENT.  State per source, device-resident, all allocated here: a zeroed history ring per channel shared by
 *   the slots, the absolute sample counter n0, and V slots {held, key, d0, g0[bands], w0[2]}, all free.  The matching below
 *   depends only on the keys and on which slots are held, so the library does it on a host-side copy of (held, key) per slot;
 *   the audio thread is its only writer.  Calling init again re-initialises the source with the new F, T, V and D.
 *   fs_reflection_render_release: history := 0 and every slot free — the next callback's voices fade in from silence (a source
 *   without fs_reflection_render_init: nothing to do, FS_OK).
 *   One callback, per row i with its voice_counts[i] entries voices[i * stride ..].  fp32 throughout; every operation is rounded
 *   on its own, in the order written (the library is built with -ffp-contract=off); numpy float32 computes the same bits.
 *     1. Match, against the slots as the previous callback left them; for an entry d1 = delay * (float)fs, g1 = band_gain,
 *        w1 = channel_gain.
 *        - A held slot whose key is among the row's entries CONTINUES: it ramps from its state (d0, g0, w0) to (d1, g1, w1).
 *        - A held slot whose key is not ENDS: d1 := d0 (the delay freezes), g1 := g0, w1 := 0.  It is free after this callback,
 *          not during it.
 *        - The entries whose key no held slot has, in list order: each STARTS on the lowest-numbered slot that was free when the
 *          callback began and has not been taken in this callback, with d0 := d1, g0 := g1, w0 := 0.  When no such slot is left
 *          the entry is DROPPED for this callback: not rendered, counted, and started by a later callback if the host still
 *          lists it and a slot is free.  A host that wants no drops gives voices = 2 x the largest number of entries it lists.
 *     2. Voice output.  For every sounding slot j (continuing, ending or starting) y_j(s, ch) is "Output s" of the direct
 *        renderer above, verbatim, with this slot's (d0, e, g0, g1): e = clamp(d1 - d0, -F/2, +F/2); cA[t] band by band
 *        ascending; a = (float)(s + 1) / (float)F; the four accumulators over t = j (mod 4) combined as
 *        (acc_0 + acc_1) + (acc_2 + acc_3); x(n) the source's shared history followed by this block.
 *     3. Sum, over the sounding slots in ascending slot number, from acc = 0: dw = w1[ch] - w0[ch]; w = w0[ch] + a * dw;
 *        acc = acc + w * y_j.  out(s, ch) = acc, not clamped.  A row without a sounding slot gives zeros.
 *     4. Afterwards a continuing or started slot holds d0 + e, g1 (0 beyond num_bands) and w1; an ended slot is free; the block
 *        enters the history; n0 += F.  rows[i] = the counts of this callback: sounding = slots rendered, started, ended, dropped.
 *   fs_reflection_render_process_batch.
 *     in  [count][frame_size * 2]  interleaved stereo, host; row i belongs to sources[i]
 *     voices [count][stride], voice_counts [count]: row i lists voice_counts[i] entries, 0 .. stride
 *     out [count][frame_size * 2]  or NULL
 *     mix [frame_size * 2]         or NULL; out == NULL && mix == NULL is FS_ERR_INVALID_ARGUMENT
 *     rows [count]                 or NULL
 *    Refusals.  Each refuses the WHOLE call before any state change or enqueue — nothing changes, out, mix and rows are not
 *    written: FS_ERR_INVALID_ARGUMENT for a NULL sources, in, voices or voice_counts; count outside
 *    1 .. FS_MAX_REFLECTION_RENDER_BATCH; stride outside 1 .. FS_MAX_REFLECTION_VOICES; a voice_counts[i] outside 0 .. stride; a
 *    key that appears twice in one row; a delay that is negative, not finite or with d1 > D; a band gain (band < num_bands) that
 *    is negative or not finite; a channel gain that is not finite; a handle that appears twice; a source without
 *    fs_reflection_render_init; sources that do not share F and T (V may differ).  FS_ERR_BAD_HANDLE for a bad handle,
 *    FS_ERR_NO_DEVICE without a device.
 *    Batch rules: 1, 2, 4 and 5 of fs_direct_render_process_batch, read for this call.  A source gives the same bits and the
 *    same state served alone, in any batch or in a permuted batch; mix is the fp32 sum in list order, computed on the device;
 *    the call runs on the reverb stream, waits for that stream only, takes no source mutex and reads no impulse response; ONE
 *    audio render thread runs all callbacks of a context (reverb, direct and reflections); staging of its own (pinned + device)
 *    grows at the first call that needs more (count x frame_size, count x stride) and a call of a shape the context has seen
 *    allocates nothing; one copy up, a number of launches that does not grow with count, one copy back, one wait.
 *   fs_source_destroy and fs_context_destroy free everything. */
#define FS_MAX_REFLECTION_VOICES        32   /* slots per source */
#define FS_MAX_REFLECTION_RENDER_BATCH 256
typedef struct fs_reflection_voice {
    uint32_t key;                     /* identity from callback to callback: fs_reflection_path.triangle */
    float    delay;                   /* s, >= 0: fs_reflection_path.delay, less whatever latency the host compensates */
    float    band_gain[FS_MAX_BANDS]; /* finite, >= 0: fs_reflection_path.reflectance; entries beyond num_bands ignored */
    float    channel_gain[2];         /* finite, any sign: the host's pan and distance law, left / right */
} fs_reflection_voice;                /* an array element: no struct_size; 48 bytes */
typedef struct fs_reflection_render_row {
    uint32_t sounding, started, ended, dropped;
} fs_reflection_render_row;           /* 16 bytes */
int fs_reflection_render_init(fs_context* ctx, fs_source src, int32_t frame_size, int32_t taps, int32_t voices, float max_delay_seconds);
int fs_reflection_render_release(fs_context* ctx, fs_source src);
int fs_reflection_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in /* [count][F * 2] */,
                                       const fs_reflection_voice* voices /* [count][stride] */, const int32_t* voice_counts /* [count] */,
                                       int32_t stride, float* out /* [count][F * 2] or NULL */, float* mix /* [F * 2] or NULL */,
                                       fs_reflection_render_row* rows /* [count] or NULL */);

/* ---- binaural voices on the audio thread (EXTENDED): every discrete path rendered from its arrival direction -------------------
 *      Not in the reference.  The reflection renderer above with the per-channel gain pair replaced by ONE scalar gain and a
 *      direction in the head frame: each ear convolves the voice with the head-related impulse response (HRIR) of the nearest
 *      direction of a host-supplied set, folded into the voice's band FIR.  Convolution is linear in the taps, so the fold is the
 *      same tap loop on a longer table, and a change of the nearest direction is a block-long crossfade between two tables —
 *      the ramp the loop already applies.  Interaural delay, head shadow and whatever else the set encodes come out of the set;
 *      without a mesh on the set (fs_hrtf_set_mesh, below) the library interpolates nothing between the set's directions.
 *   Head frame.  x forward, y right, z up (the reference's Unreal convention); ear 0 is the left ear, ear 1 the right.
 *   fs_hrtf_set.  n = directions, H = taps, dirs [n][3], hrir [n][2][H] (direction, ear, tap).  Accepted when struct_size is this
 *   library's, 1 <= n <= FS_MAX_HRTF_DIRECTIONS, 1 <= H <= FS_MAX_HRTF_TAPS, sample_rate == the context's, dirs and hrir are not
 *   NULL, every direction is finite with |x^2 + y^2 + z^2 - 1| <= 1e-3 (in double) and every tap is finite: otherwise
 *   FS_ERR_INVALID_ARGUMENT, and a refused call changes nothing.  desc == NULL clears the set.  The audio thread's contract: not
 *   concurrent with a callback.  The call waits for the reverb stream, uploads the set in one copy and frees every held binaural
 *   slot of every source of the context; the histories are kept.  So the next callback's voices START — they fade in from
 *   silence over one block — and nothing ever ramps from an index of the old set.  The call, whether given a set or NULL, also
 *   drops the mesh (fs_hrtf_set_mesh).  (A HIP failure after the upload is no refusal:
 *   it is reported with the new set in force and every source's slots freed on the host's copy, so every voice still starts.)  A source initialised under a set of another H
 *   stays initialised; fs_binaural_render_process_batch refuses it while D + Tc + 1 + F exceeds its ring or Tc exceeds
 *   FS_DIRECT_RENDER_MAX_TAPS (below), and fs_binaural_render_init sizes it anew.
 *   fs_hrtf_info: *directions = n and *taps = H of the set in force, 0 and 0 without one (either pointer may be NULL).
 *   fs_hrtf_spherical_head.  A set for hosts that have none; host only, no context, no device.  A MODEL: a rigid sphere's
 *   interaural delay and level difference, NO pinna — no elevation cue and no front/back cue beyond what the delay gives.
 *   a = radius_cm, c = sound_speed_cm_s (real physics, cm/s: NOT the trace's dist_divisor time axis), fs = sample_rate; suggested
 *   a = FS_HRTF_DEFAULT_RADIUS_CM, c = FS_HRTF_DEFAULT_SOUND_SPEED_CM_S.  Computed in double, rounded to float once.
 *     Directions, k = 0 .. n-1:  z = 1 - (2k + 1) / n;  rho = sqrt(1 - z^2);  phi = k pi (3 - sqrt 5);
 *       p_k = (rho cos phi, rho sin phi, z)    (a Fibonacci spiral from the zenith down).
 *     Per ear, axis e = (0, -1, 0) left, (0, +1, 0) right:  theta = acos(clamp(p . e, -1, 1)).
 *       Onset (Woodworth's delay, offset so that it is never negative):
 *         tau = (a / c) (1 - cos theta) for theta <= pi / 2, else tau = (a / c) (1 + theta - pi / 2).
 *       Shadow (Brown and Duda's one-pole, one-zero filter):  alpha = (1 + alpha_min / 2) + (1 - alpha_min / 2) cos(theta pi /
 *         theta_min), alpha_min = 0.1, theta_min = 5 pi / 6;  kappa = fs a / c;  g = the impulse response of the bilinear
 *         transform ((1 + alpha kappa) + (1 - alpha kappa) z^-1) / ((1 + kappa) + (1 - kappa) z^-1):
 *         g[0] = b0, g[1] = b1 - a1 g[0], g[m] = -a1 g[m-1], with b0 = (1 + alpha kappa) / (1 + kappa), b1 = (1 - alpha kappa) /
 *         (1 + kappa), a1 = (1 - kappa) / (1 + kappa).
 *       Taps:  i = floor(tau fs), f = tau fs - i;  h[k] = (1 - f) g[k - i] + f g[k - i - 1], g = 0 at negative indices.
 *     FS_ERR_INVALID_ARGUMENT: dirs or hrir NULL, sample_rate < 1, a or c not finite or not > 0, n outside
 *     1 .. FS_MAX_HRTF_DIRECTIONS, H outside 1 .. FS_MAX_HRTF_TAPS, or H < ceil((a / c) (1 + pi / 2) fs) + 2 (the latest onset
 *     plus the filter's first two taps would not fit).
 *   The mesh (optional): a triangulation of the set's directions, over which a voice's HRIR is the barycentric blend of the three
 *   at the corners of the spherical triangle its direction falls in — a source walking round the listener no longer hops from one
 *   measured direction to the next.  Without a mesh everything above and below is as it stands, to the bit.  The blend is of the
 *   time-domain HRIRs as given: neighbours whose onsets differ comb (two half-height arrivals, not one in between) unless the
 *   set carries its onsets apart (fs_hrtf_set_onsets, below); near-field sets and more than one mesh per context are not offered.
 *   fs_hrtf_mesh_rows.  Host only, no context, no device: the validator and the one definition of the mesh data.  dirs [n][3],
 *   tri [m][3] indices into dirs.  Accepted when 4 <= n <= FS_MAX_HRTF_DIRECTIONS and m == 2n - 4; every index lies in 0 .. n-1;
 *   the three indices of a triangle are distinct; every directed edge a->b occurs in exactly one triangle and b->a in exactly one
 *   (a closed, consistently oriented surface); every direction is a corner of some triangle; and for every triangle (a, b, c)
 *   det = p_a . (p_b x p_c) >= 1e-6, in double from the float directions as given (counter-clockwise seen from outside, the
 *   origin on its inner side).  Then, in double, each component rounded to float once:
 *     r_0 = (p_b x p_c) / det,  r_1 = (p_c x p_a) / det,  r_2 = (p_a x p_b) / det   into rows [m][3][3],
 *   so that g_i = r_i . d are the coefficients of d = sum g_i p_i.  rows == NULL only validates.  Anything else (a NULL dirs or
 *   tri among it): FS_ERR_INVALID_ARGUMENT, and nothing is written.
 *   fs_hrtf_triangulate.  Host only.  The convex hull of the directions — for points on a sphere the Delaunay triangulation — as
 *   such a mesh: *m = 2n - 4 triangles into tri [cap][3].  Computed in double.  Where four or more directions lie on one circle
 *   (a lat-long grid) the split of their facet is free: the output is specified by its properties — it passes fs_hrtf_mesh_rows
 *   and no direction lies above a triangle's plane — not to the bit.  FS_ERR_INVALID_ARGUMENT, nothing written: dirs, tri or m
 *   NULL, n outside 4 .. FS_MAX_HRTF_DIRECTIONS, cap < 2n - 4, a component that is not finite, or a result fs_hrtf_mesh_rows
 *   would refuse (all directions in one hemisphere or on one great circle, a direction given twice).
 *   fs_hrtf_mesh_locate.  Host only.  The rule the callback applies on the device, by the same function: fp32, every operation
 *   rounded on its own, in the order written.  rows [m][3][3] as fs_hrtf_mesh_rows gives them, m >= 1, d [3] any length.
 *     1. For each triangle j: g_i = (d.x r_i.x + d.y r_i.y) + d.z r_i.z, i = 0, 1, 2;  mu_j = g_0; if (g_1 < mu_j) mu_j = g_1;
 *        if (g_2 < mu_j) mu_j = g_2.
 *     2. *t = the LOWEST j that maximises mu_j: from best = -infinity and t = 0, j ascending, mu_j replaces best where
 *        mu_j > best (an equal later one does not; one that is not a number never does).
 *     3. c_i = g_i > 0 ? g_i : 0.0f (of triangle t);  s = (c_0 + c_1) + c_2;  b_i = c_i / s;  if !(s > 0): b = (1, 0, 0).
 *     FS_ERR_INVALID_ARGUMENT, nothing written: a NULL pointer or m < 1.
 *   fs_hrtf_set_mesh.  Needs a set in force.  tri [m][3] is validated by fs_hrtf_mesh_rows' code against the set's directions;
 *   otherwise (or m < 0, or without a set) FS_ERR_INVALID_ARGUMENT, and a refused call changes nothing.  tri == NULL or m == 0
 *   clears the mesh.  Either way the call then behaves as fs_hrtf_set: not concurrent with a callback; it waits for the reverb
 *   stream, uploads the triangles and their rows in one copy and frees every held binaural slot of every source, the histories
 *   kept — every voice starts from silence, and nothing ramps from an index of the other mode.  Tc and the ring sizes do not
 *   depend on the mesh.  fs_hrtf_mesh_info: *triangles = m of the mesh in force, 0 without one (the pointer may be NULL).
 *   Onsets (optional).  A set in force may carry onsets o[j][ear], one float per direction and ear, in samples; hrir[j][ear][.]
 *   is then read as the HRIR with that onset removed ("aligned"), and a voice's HRIR is the aligned one — the nearest, or with a
 *   mesh the blend — delayed by the voice's own onset — the nearest's, or the blend of the corners' onsets: the interaural delay
 *   glides with the direction where blending the HRIRs as given would cross-fade between two arrivals.  Without onsets everything
 *   above and below is as it stands, to the bit.  With onsets in force:
 *     omax = the largest onset of the set (a float);  O = (int)omax + 1;  He = H + O;  and Tc = T + He - 1 wherever Tc stands:
 *     the ring sizing of fs_binaural_render_init, the refusal of a source whose ring the set has outgrown, the folded tables and
 *     the render pass.
 *     The delay of end A, ear `ear`:  nearest mode: tauA = o[qA][ear];  with a mesh, (v_0, v_1, v_2) = tri[tA]:
 *       tauA = (bA_0 * o[v_0][ear] + bA_1 * o[v_1][ear]) + bA_2 * o[v_2][ear];
 *     then  if (tauA > omax) tauA = omax  (the weights sum to 1 only within 2 ulp: the clamp keeps the last tap inside He).  All
 *     terms are >= 0, so tauA >= 0.
 *     The delayed HRIR (fs_hrtf_delay: host only, the same function as the kernel's; fp32, every operation rounded on its own):
 *       i = (int)tau;  f = tau - (float)i;  g = 1.0f - f;
 *       hd[k] = g * x(k - i) + f * x(k - i - 1),  k = 0 .. He-1,  x(j) = hA[j] for 0 <= j < H, else 0.0f,
 *     with hA = h[qA][ear] in nearest mode, or rule 3''s blend, rounded as there, with a mesh: the linear fractional delay
 *     fs_hrtf_spherical_head specifies for its own onsets.  Rules 3 and 3' then read hd[k] in h's place, k up to min(He - 1, u).
 *     Equal q, or equal (t, b) bits, give equal tau bits: where one fold serves both ends it still does.  A change of direction
 *     stays a block-long ramp between two tap tables, not a delay that glides inside the block.
 *   fs_hrtf_set_onsets.  Needs a set in force.  onsets [n][2]; every onset finite and >= 0, and H + (int)omax + 1 <=
 *   FS_MAX_HRTF_TAPS: otherwise (or without a set) FS_ERR_INVALID_ARGUMENT, and a refused call changes nothing.  onsets == NULL
 *   clears them.  Either way the call then behaves as fs_hrtf_set_mesh: not concurrent with a callback; it waits for the reverb
 *   stream, uploads in one copy and frees every held binaural slot of every source, the histories kept.  It does not drop the
 *   mesh, and fs_hrtf_set_mesh does not drop the onsets; fs_hrtf_set, given a set or NULL, drops both.  A source initialised
 *   before the call is refused by the callback while its ring is too small for the new Tc, exactly as after a set of another H.
 *   fs_hrtf_onsets_info: *installed = 1 with onsets in force, else 0; *extra_taps = O, 0 without (either pointer may be NULL).
 *   fs_hrtf_delay.  Host only.  out[0 .. He) = hd of h[0 .. H) and tau by the rule above.  FS_ERR_INVALID_ARGUMENT, nothing
 *   written: a NULL pointer, H < 1, tau not finite or negative, or He < H + (int)tau + 1.
 *   fs_hrtf_split_onsets.  Host only: for hosts whose set comes without delays.  hrir [n][2][H]; threshold in (0, 1], lead >= 0,
 *   n >= 1, H >= 1, no NULL pointer (else FS_ERR_INVALID_ARGUMENT, nothing written).  Per (direction, ear): peak = max |h[k]|;
 *   k0 = the lowest k with |h[k]| >= threshold * peak (an fp32 product); onset = (float)max(k0 - lead, 0); aligned[k] =
 *   h[k + onset] while k + onset < H, else 0.0f.  An all-zero HRIR gets onset 0.  aligned may be hrir.  Integer onsets only —
 *   what a mesh blends between them is fractional.
 *   fs_hrtf_spherical_head_split.  fs_hrtf_spherical_head with its two halves handed out apart: hrir[k] = g[k], the shadow
 *   filter alone, and onsets [n][2] = tau fs; in double, each value rounded to float once.  Its refusals, with onsets NULL among
 *   them and 2 <= H <= FS_MAX_HRTF_TAPS in the place of the bound on H (the onset needs no taps).
 *   fs_binaural_render_init.  Needs a set in force.  F, T, D and V under fs_reflection_render_init's limits with Tc = T + H - 1
 *   wherever the ring is sized: 16 <= F <= 16384; T odd, 1 .. FS_DIRECT_RENDER_MAX_TAPS; Tc <= FS_DIRECT_RENDER_MAX_TAPS; the ring
 *   is the smallest power of two >= D + Tc + 1 + F floats and D + Tc + 1 + F <= 2^20; edges in force inside (0, fs / 2);
 *   1 <= V <= FS_MAX_REFLECTION_VOICES: otherwise FS_ERR_INVALID_ARGUMENT.  The state is the binaural renderer's own — a source may
 *   hold direct, reflection and binaural state side by side: a zeroed history ring per channel, n0, and V slots {held, key, d0,
 *   g0[bands], w0, q0}, all free; the host-side copy of (held, key) as above.  fs_binaural_render_release: history := 0, every slot
 *   free (a source without fs_binaural_render_init: nothing to do, FS_OK).
 *   One callback, per row.  fp32 throughout, every operation rounded on its own, in the order written.
 *     1. Match.  Rule 1 of the reflection renderer, verbatim, with w1 = gain (one scalar) and w0 := 0 at a start.
 *     2. HRIR index.  For an entry with direction d: q1 = the LOWEST index j that maximises (d.x p_j.x + d.y p_j.y) + d.z p_j.z
 *        over the set's directions (d need not be unit).  A slot holds q0, the index its last callback ended with.  A starting
 *        slot takes q0 := q1; an ending slot q1 := q0.
 *     3. Taps.  fA[t], A = 0, 1, t = 0 .. T-1: the direct renderer's cA[t] from g0 and g1.  Per ear, u = 0 .. Tc-1:
 *        CA[u] = the sum from acc = 0 over k ascending from max(0, u - T + 1) to min(H - 1, u) of acc = acc + h[qA][ear][k] *
 *        fA[u - k];  dC[u] = C1[u] - C0[u].
 *     4. Voice output.  "Output s" of the direct renderer with Tc taps and the coefficient C0[u] + a * dC[u]: the same delay,
 *        slew limit (e = clamp(d1 - d0, -F/2, +F/2)) and four accumulators.  Ear ch reads input channel ch of the source's shared
 *        history followed by this block: a mono source is given in both channels.
 *     5. Sum, over the sounding slots in ascending slot number, from acc = 0: dw = w1 - w0; w = w0 + a * dw; acc = acc + w * y_j —
 *        the same scalar w for both ears.  Not clamped.  A row without a sounding slot gives zeros.
 *     6. Afterwards a continuing or started slot holds d0 + e, g1 (0 beyond num_bands), w1 and q1; an ended slot is free; the
 *        block enters the history; n0 += F.  rows[i] as the reflection renderer's.
 *     With a mesh in force rules 2, 3 and 6 read:
 *     2'. Locate.  An entry with direction d gets (t1, b1[3]) from fs_hrtf_mesh_locate on the mesh's rows.  A slot holds
 *        (t0, b0[3]) from the end of its last callback.  A starting slot takes (t0, b0) := (t1, b1); an ending slot
 *        (t1, b1) := (t0, b0).
 *     3'. Taps.  With (v_0, v_1, v_2) = tri[tA], per ear:  hA[k] = (bA_0 * h[v_0][ear][k] + bA_1 * h[v_1][ear][k]) +
 *        bA_2 * h[v_2][ear][k];  CA[u] as in rule 3 with hA[k] in the place of h[qA][ear][k].
 *     6'. A continuing or started slot holds (t1, b1) in q1's place.
 *     (Where t0 == t1, b0 and b1 have the same bits and so have g0 and g1, C1 has C0's bits either way.)
 *     Consequence: with a set of H = 1 whose taps are all 1.0f the output equals fs_reflection_render_process_batch's with
 *     channel_gain = (gain, gain).  The output is late by (T - 1) / 2 samples plus whatever onset the set's HRIRs carry — with
 *     onsets in force, plus the delayed HRIR's onset tauA.
 *   fs_binaural_render_process_batch.  Arguments, refusals and batch rules of fs_reflection_render_process_batch, read for this
 *   call, and further FS_ERR_INVALID_ARGUMENT for: no set in force; a gain that is not finite; a direction with a component that
 *   is not finite or with all three zero; a source without fs_binaural_render_init; sources that do not share F and T (hence Tc);
 *   a source whose ring the set in force has outgrown (fs_hrtf_set above).  Staging of its own (pinned + device), which holds the
 *   folded tables {C0, dC} [sum of the listed sources' V][2][Tc] beside the rest and grows at the first call that needs more; a call
 *   of a shape the context has seen allocates nothing (with a mesh the staging also holds what the locate pass finds; a shape
 *   is a shape under one mode).  One copy up, four launches whatever the count (plan, taps, render, mix) — five with a mesh
 *   (locate first: one wave of 64 lanes per voice with an entry, striding over the triangles) —
 *   one copy back, one wait on the reverb stream.  ONE audio render thread runs all callbacks of a context.
 *   A key for the direct sound: FS_BINAURAL_DIRECT_KEY, a first-order key (a triangle index) no scene of fewer than 2^29 - 1
 *   triangles uses.
 *   fs_source_destroy and fs_context_destroy free everything. */
#define FS_MAX_HRTF_DIRECTIONS 4096
#define FS_MAX_HRTF_TAPS       512
#define FS_MAX_HRTF_TRIANGLES (2 * FS_MAX_HRTF_DIRECTIONS - 4)
#define FS_HRTF_DEFAULT_RADIUS_CM          8.75f
#define FS_HRTF_DEFAULT_SOUND_SPEED_CM_S   34300.0f
#define FS_BINAURAL_DIRECT_KEY 0x1FFFFFFFu
typedef struct fs_hrtf_desc {
    uint32_t struct_size;
    int32_t  directions;              /* n */
    int32_t  taps;                    /* H */
    int32_t  sample_rate;             /* the rate the taps were sampled at: the context's */
    const float* dirs;                /* [n][3] unit vectors, head frame */
    const float* hrir;                /* [n][2][H]: direction, ear (0 left, 1 right), tap */
} fs_hrtf_desc;
typedef struct fs_binaural_voice {
    uint32_t key;                     /* identity from callback to callback, as fs_reflection_voice.key */
    float    delay;                   /* s, >= 0: the path's delay, less whatever latency the host compensates */
    float    band_gain[FS_MAX_BANDS]; /* finite, >= 0; entries beyond num_bands ignored */
    float    gain;                    /* finite, any sign: the host's distance law */
    float    direction[3];            /* head frame, towards where the sound arrives from: finite, not all zero, any length */
} fs_binaural_voice;                  /* an array element: no struct_size; 56 bytes */
typedef struct fs_binaural_render_row {
    uint32_t sounding, started, ended, dropped;
} fs_binaural_render_row;             /* 16 bytes */
int fs_hrtf_set(fs_context* ctx, const fs_hrtf_desc* desc /* NULL: clear */);
int fs_hrtf_info(fs_context* ctx, int32_t* directions, int32_t* taps);
int fs_hrtf_spherical_head(int32_t sample_rate, float radius_cm, float sound_speed_cm_s, int32_t directions, int32_t taps,
                           float* dirs /* [directions][3] */, float* hrir /* [directions][2][taps] */);
int fs_hrtf_triangulate(const float* dirs /* [n][3] */, int32_t n, int32_t* tri /* [cap][3] */, int32_t cap, int32_t* m);
int fs_hrtf_mesh_rows(const float* dirs /* [n][3] */, int32_t n, const int32_t* tri /* [m][3] */, int32_t m, float* rows /* [m][3][3] or NULL */);
int fs_hrtf_mesh_locate(const float* rows /* [m][3][3] */, int32_t m, const float d[3], int32_t* t, float b[3]);
int fs_hrtf_set_mesh(fs_context* ctx, const int32_t* tri /* [m][3]; NULL or m == 0: clear */, int32_t m);
int fs_hrtf_mesh_info(fs_context* ctx, int32_t* triangles);
int fs_hrtf_set_onsets(fs_context* ctx, const float* onsets /* [n][2]; NULL: clear */);
int fs_hrtf_onsets_info(fs_context* ctx, int32_t* installed, int32_t* extra_taps /* O, 0 without */);
int fs_hrtf_delay(const float* h /* [H] */, int32_t H, float tau, float* out /* [He] */, int32_t He);
int fs_hrtf_split_onsets(const float* hrir /* [n][2][H] */, int32_t n, int32_t H, float threshold, int32_t lead,
                         float* aligned /* [n][2][H], may be hrir */, float* onsets /* [n][2] */);
int fs_hrtf_spherical_head_split(int32_t sample_rate, float radius_cm, float sound_speed_cm_s, int32_t directions, int32_t taps,
                                 float* dirs /* [directions][3] */, float* hrir /* [directions][2][taps] */, float* onsets /* [directions][2] */);
int fs_binaural_render_init(fs_context* ctx, fs_source src, int32_t frame_size, int32_t taps, int32_t voices, float max_delay_seconds);
int fs_binaural_render_release(fs_context* ctx, fs_source src);
int fs_binaural_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in /* [count][F * 2] */,
                                     const fs_binaural_voice* voices /* [count][stride] */, const int32_t* voice_counts /* [count] */,
                                     int32_t stride, float* out /* [count][F * 2] or NULL */, float* mix /* [F * 2] or NULL */,
                                     fs_binaural_render_row* rows /* [count] or NULL */);

/* ---- ambisonic voices on the audio thread (EXTENDED): every discrete path rendered into a soundfield -----------------------------
 *      Not in the reference.  The reflection renderer above with the per-channel gain pair replaced by ONE scalar gain and a
 *      direction in the head frame, as the binaural renderer's entries, and the two output channels replaced by the
 *      C = (order + 1)^2 channels of an ambisonic bus: ACN channel order, SN3D normalisation (AmbiX), orders 0 .. 3.  The bus feeds
 *      loudspeakers through a decoder, rotates with one small matrix per order — a head tracker may run faster than the audio
 *      block — and decodes to a host's own binaural decoder.  Rotation and decoding stay the host's; the library renders the voice
 *      bank: the delay with its Doppler shift, the band FIR, the keyed one-block fades.  A voice's filter is evaluated ONCE, not
 *      once per output channel, and fanned out to the C channels by ramping gains.
 *   Signal.  A point source is mono: a source has ONE history ring, and x(n) = 0.5f * (in[2n] + in[2n + 1]) is what enters it.
 *   A mono source given in both channels — what the other renderers ask for — is x to the bit.
 *   Encoding, of a direction d in the head frame (x forward, y right, z up; AmbiX has y to the left, so y is negated).  fp32,
 *   every operation rounded on its own, in the order written; division and square root correctly rounded:
 *     len = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z);  x = d.x/len;  y = -(d.y/len);  z = d.z/len;  xx = x*x;  yy = y*y;  zz = z*z;
 *     K3 = (float)sqrt(3.0), K3h = (float)(sqrt(3.0)/2), K58 = (float)sqrt(5.0/8), K15 = (float)sqrt(15.0),
 *     K38 = (float)sqrt(3.0/8), K15h = (float)(sqrt(15.0)/2)   (the double values rounded to float once)
 *     Y0 = 1
 *     Y1 = y               Y2 = z                           Y3 = x
 *     Y4 = K3*(x*y)        Y5 = K3*(y*z)                    Y6 = 1.5f*zz - 0.5f    Y7 = K3*(x*z)    Y8 = K3h*(xx - yy)
 *     Y9 = K58*(y*(3.0f*xx - yy))    Y10 = K15*((x*y)*z)    Y11 = K38*(y*(5.0f*zz - 1.0f))    Y12 = z*(2.5f*zz - 1.5f)
 *     Y13 = K38*(x*(5.0f*zz - 1.0f)) Y14 = K15h*(z*(xx - yy))   Y15 = K58*(x*(xx - 3.0f*yy))
 *   These are sqrt((2 - delta_m0) (n - |m|)! / (n + |m|)!) P_n^|m|(z) {cos, sin}(|m| az) without the Condon-Shortley phase, channel
 *   n (n + 1) + m; each order's squares sum to 1.  A direction is legal when its components are finite and its fp32 squared length
 *   (d.x*d.x + d.y*d.y) + d.z*d.z is finite and lies in [1e-30f, 1e30f].
 *   fs_ambisonic_encode writes Y_0 .. Y_{C-1} of a direction; host only, no context, no device: for hosts that encode other beds
 *   into the same bus.  The plan pass on the device gives the same bits.  FS_ERR_INVALID_ARGUMENT: order outside
 *   0 .. FS_MAX_AMBISONIC_ORDER, direction or out NULL, a direction that is not legal.
 *   fs_ambisonic_render_init.  F, T, D and V under fs_reflection_render_init's limits, 0 <= order <= FS_MAX_AMBISONIC_ORDER:
 *   otherwise FS_ERR_INVALID_ARGUMENT.  The state is the ambisonic renderer's own — a source may hold direct, reflection, binaural
 *   and ambisonic state side by side: ONE zeroed history ring (the smallest power of two >= D + T + 1 + F floats), n0, and V slots
 *   {held, key, d0, g0[bands], w0[16]}, all free; the host-side copy of (held, key) as the reflection renderer's.  Calling init
 *   again re-initialises the source with the new F, T, V, D and order.  fs_ambisonic_render_release: history := 0, every slot free
 *   (a source without fs_ambisonic_render_init: nothing to do, FS_OK).
 *   One callback, per row.  fp32 throughout, every operation rounded on its own, in the order written.
 *     1. Match.  Rule 1 of the reflection renderer, verbatim, with w1[c] = gain * Y_c(direction) for c < C — the aim of an entry —
 *        w1 := 0 at an END and w0 := 0 at a START.
 *     2. Voice output.  For every sounding slot j, y_j(s) is "Output s" of the direct renderer, verbatim, on x(n) — the source's
 *        one history followed by this block's downmix — with this slot's (d0, e, g0, g1).  One value per sample, not one per
 *        channel.
 *     3. Sum, over the sounding slots in ascending slot number, from acc = 0, per channel c < C: dw = w1[c] - w0[c];
 *        w = w0[c] + a * dw;  acc = acc + w * y_j.  out(s, c) = acc, not clamped.  A row without a sounding slot gives zeros.
 *     4. Afterwards a continuing or started slot holds d0 + e, g1 (0 beyond num_bands) and w1; an ended slot is free; the block's
 *        downmix enters the history; n0 += F.  rows[i] as the reflection renderer's.
 *     Consequences.  At order 0 with a mono source in both channels the output equals channel 0 of
 *     fs_reflection_render_process_batch with channel_gain = (gain, gain).  At any order channels (c, c') equal the reflection
 *     renderer's two channels with channel_gain = (gain * Y_c, gain * Y_c') from fs_ambisonic_encode, to the bit.
 *   fs_ambisonic_render_process_batch.
 *     in  [count][frame_size * 2]  interleaved stereo, host; row i belongs to sources[i]
 *     out [count][frame_size * C]  or NULL; interleaved by sample: element s * C + c
 *     mix [frame_size * C]         or NULL; out == NULL && mix == NULL is FS_ERR_INVALID_ARGUMENT
 *   voices, voice_counts, stride and rows as fs_reflection_render_process_batch's.  Its refusals and batch rules, read for this
 *   call, and further FS_ERR_INVALID_ARGUMENT for: a gain that is not finite; a direction that is not legal (above); a source
 *   without fs_ambisonic_render_init; sources that do not share F, T and order.  A refused call changes nothing.  A source gives
 *   the same bits and the same state served alone, in any batch or in a permuted batch; mix is the fp32 sum in list order,
 *   computed on the device, and with out == NULL only mix comes back — at order 3 a row of out is 8 times a stereo row, so a host
 *   that wants the bus asks for mix alone.  Staging of its own (pinned + device), grown at the first call that needs more; a call
 *   of a shape the context has seen allocates nothing.  One copy up, three launches whatever the count (plan, render, mix), one
 *   copy back, one wait on the reverb stream.  ONE audio render thread runs all callbacks of a context.
 *   The output is late by (T - 1) / 2 samples.  Not here: a decoder or rotator, orders above 3.  The late field of this bus is
 *   fs_reverb_soundfield_process_batch's (below): a host sums the two mix rows.
 *   fs_source_destroy and fs_context_destroy free everything. */
#define FS_MAX_AMBISONIC_ORDER 3
typedef fs_binaural_voice fs_ambisonic_voice;      /* key, delay, band_gain, gain, direction (head frame): 56 bytes */
typedef struct fs_ambisonic_render_row {
    uint32_t sounding, started, ended, dropped;
} fs_ambisonic_render_row;            /* 16 bytes */
int fs_ambisonic_encode(int32_t order, const float* direction /* [3] */, float* out /* [(order + 1)^2] */);
int fs_ambisonic_render_init(fs_context* ctx, fs_source src, int32_t frame_size, int32_t taps, int32_t voices, float max_delay_seconds,
                             int32_t order);
int fs_ambisonic_render_release(fs_context* ctx, fs_source src);
int fs_ambisonic_render_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in /* [count][F * 2] */,
                                      const fs_ambisonic_voice* voices /* [count][stride] */, const int32_t* voice_counts /* [count] */,
                                      int32_t stride, float* out /* [count][F * C] or NULL */, float* mix /* [F * C] or NULL */,
                                      fs_ambisonic_render_row* rows /* [count] or NULL */);

/* ---- soundfield late reverb (EXTENDED; DESIGN.md section 8, "Soundfield late reverb"): the late field on the ambisonic bus ----
 * A partitioned reverb source initialised with the SOUNDFIELD convolves its mono downmix with one impulse response per channel of
 * an ACN/SN3D bus of C = (order + 1)^2 channels.  A diffuse field has no direction, only a covariance across the channels, and that
 * is diagonal: with unit power in W (channel 0), every channel of degree l carries power 1 / (2 l + 1), and distinct channels are
 * uncorrelated.  So channel c (degree l(c) = floor(sqrt(c))) gets an IR of its own, built the way the ear IRs are — band envelope
 * times band-limited noise carrier, summed over the bands — with carriers that are independent from channel to channel.  Nothing
 * in the trace, the reconstruct or the publish path changes.
 *
 * The carriers are context-wide and use the bands, the bin assignment and K (the smallest power of two >= num_samples) of
 * FS_FLAG_SPECTRAL_IR, fs_set_band_edges included.  For channel c < C and bin k in [1, K/2):
 *   1. seed_c = 0x5EED + (c << 32), in 64 bits: channel 0 has the spectral IR's phases, the streams seed_c + k of two channels
 *      never meet, and none meets the ears' side seed 0x5EED0EA2 + k;
 *      phi_{c,k} = 2 pi (splitmix64(seed_c + k) >> 40) 2^-24;
 *   2. the spectrum of (c, band b) is exp(i phi_{c,k}) on the band's bins, cosine and sine formed in double and rounded to float once;
 *   3. r_{c,b} = its real inverse transform (the spectral IR's inverse passes);
 *   4. g_{c,b} = sqrt(N / sum_{n<N} r_{c,b}[n]^2), the sum in double; car_{c,b} = g_{c,b} r_{c,b}: unit mean power over the IR.
 * Per source, env_b = the source's device-resident band row b (what fs_copy_band_impulse_response copies), whatever flags the
 * reconstruct had; after fs_set_impulse_response every band row is the installed IR:
 *   5. m = 0.0f;  for (b = 0; b < B; ++b) m = m + env_b[n] * car_{c,b}[n];      fp32, no contraction, ascending b
 *      m = m * (1.0f / sqrtf((float)B));
 *      h_c[n] = m * w_l;      w_l = 1.0f / sqrtf((float)(2 l(c) + 1)), w_0 = 1.0f exactly.
 * Consequence: h_0 has the same bits as h_L of the two-ear reverb with an ear set of radius_cm = 0 on the same band rows.
 * The signal: a point source is mono, as in the ambisonic renderer — d(n) = 0.5f * (in[2n] + in[2n + 1]) is what the source's
 * history holds.  The callback gives out(s, c) = (h_c * u)[s], u = the history followed by this block's d; interleaved by sample,
 * element s * C + c, like the ambisonic renderer's rows.  Unlike fs_reverb_process_batch the output is NOT clamped (a bus is
 * summed and decoded before it reaches a converter; the +-1 clamp is the reference's stereo callback's), there is no bypass row
 * (no apply_reverb), and flags must be 0 (FS_REVERB_LITERAL_TAIL is a reference quirk of the stereo path).
 * The engine is the partitioned one: channels 2q and 2q + 1 ride in one complex IR, G_{q,p} = FFT_N(h_{2q} + i h_{2q+1}) per
 * partition p, P = ceil(C / 2) pairs (at odd C the last pair's imaginary part is zero); the mono window is transformed once,
 * every window spectrum is read once for all P pairs, and each pair's inverse gives channel 2q in its real and channel 2q + 1 in
 * its imaginary part.  All of fs_reverb_set_crossfade holds with "the IR" read as the C-tuple.
 *
 * fs_reverb_soundfield_set (game thread, never concurrent with a callback; order -1: clear) builds [C][B][carrier_stride] on the
 * compute stream and waits for it (32 MB at order 3, 8 bands and one second).  The band edges in force must give every band a bin
 * (FS_FLAG_SPECTRAL_IR's condition and text).  Installing the order already installed is FS_OK and changes nothing; clearing, or
 * installing another order, is FS_ERR_INVALID_ARGUMENT while a source is initialised with the soundfield.  fs_set_band_edges
 * with a set installed rebuilds it, and every soundfield source takes again at its next callback (through its crossfade, if it
 * has one).  fs_reverb_soundfield_info: the order installed (-1: none).
 * fs_reverb_set_soundfield records the choice like fs_reverb_set_ears: it takes effect at the source's next fs_reverb_init, which
 * is FS_ERR_INVALID_ARGUMENT with the soundfield on when the source's engine is not FS_REVERB_ENGINE_PARTITIONED, when no set is
 * installed, or when ears are on as well (the message says which).  That init allocates everything — [P][K][N] spectra per IR copy
 * and the state of one mono window — so the callback allocates nothing.
 * fs_reverb_soundfield_process_batch: the rules of fs_reverb_process_batch, read for rows of F * C floats.
 *     in  [count][frame_size * 2]  interleaved stereo, host; row i belongs to sources[i]
 *     out [count][frame_size * C]  or NULL
 *     mix [frame_size * C]         or NULL; out == NULL && mix == NULL is FS_ERR_INVALID_ARGUMENT
 *   One set of launches whatever the count; 1 <= count <= FS_MAX_REVERB_BATCH and no handle twice; every source initialised with
 *   the soundfield at one frame size, else FS_ERR_INVALID_ARGUMENT — as is a soundfield source listed in fs_reverb_process or
 *   fs_reverb_process_batch.  A refused call changes nothing.  A source gives the same bits alone, in any batch and in a permuted
 *   batch; mix is the fp32 sum in list order, computed on the device, and with out == NULL only mix comes back — at order 3 a row
 *   of out is 8 times a stereo row, so a host that wants the bus asks for mix alone and adds it to the ambisonic renderer's mix.
 *   Reverb stream, ONE audio render thread, the per-source lock held only while work is enqueued; staging of its own, and a call of
 *   a shape the context has seen allocates nothing.
 * LATENCY: the ambisonic voices are late by (T - 1) / 2 samples and this reverb is not.  Aligning the two stays the host's, as the
 * direct renderer's text says for `delay`.
 * fs_reverb_copy_soundfield_impulse_responses (game thread, ordered like fs_copy_band_impulse_response; needs an installed set,
 * not fs_reverb_init) copies h_c, c < C, of the source's newest device-resident IR into out [C][n], n = fs_num_samples — for hosts
 * with a convolver of their own.  Not here: a directional late field, a decoder or rotator, the direct engine, per-source carrier
 * sets, orders above 3. */
int fs_reverb_soundfield_set(fs_context* ctx, int32_t order /* 0 .. FS_MAX_AMBISONIC_ORDER; -1: clear */);
int fs_reverb_soundfield_info(fs_context* ctx, int32_t* order, int32_t* installed); /* any pointer may be NULL */
int fs_reverb_set_soundfield(fs_context* ctx, fs_source src, int32_t on);
int fs_reverb_copy_soundfield_impulse_responses(fs_context* ctx, fs_source src, float* out /* [C][n] */, int32_t n);
int fs_reverb_soundfield_process_batch(fs_context* ctx, const fs_source* sources, int32_t count, const float* in /* [count][F * 2] */,
                                       float* out /* [count][F * C] or NULL */, uint32_t flags /* 0 */, float* mix /* [F * C] or NULL */);

/* ---- row f4: frequency-dependent material response of one audio block ------------------------------------
 *      UMaterialAcousticProcessor::ApplyMaterialFD (Private/MaterialAcousticProcessor.cpp:8-107, MAP.cpp):
 *      N = next power of two >= L (:15-16); forward real FFT of the zero-padded block (:29-47); per bin
 *      Refl = 1 - absorption, transmission clamped so Refl + tau <= 1, specular = Refl*(1 - scattering),
 *      diffuse = Refl*scattering, transmitted = tau (:51-72); three inverse FFTs scaled by 1/N (:75-92).
 *      The three response curves (FMaterialAcousticFD, MaterialAcousticProcessor.h:24-37) must each hold
 *      num_responses == N/2 + 1 values, otherwise FS_ERR_SIZE_MISMATCH (the reference logs the error and
 *      returns empty outputs, :20-26).  in and the three outputs are host arrays of L floats. */
int fs_apply_material_fd(fs_context* ctx, const float* in, int32_t L, const float* absorption, const float* transmission,
                         const float* scattering, int32_t num_responses, float* specular, float* diffuse,
                         float* transmitted);

/* ---- measurement --------------------------------------------------------------------------------- */
/* HIP events on the context's stream: 0 = off, 1 = around the dominant (walk) kernel only, 2 = every kernel,
 * 3 = level 2 + the kernels count the node / triangle records they fetch (slower: not for timed frames) */
int fs_set_profiling(fs_context* ctx, int32_t level);
/* level 1 only: put the event pair around every n-th frame (default 1 = every frame).  An event pair costs a frame a few
 * microseconds of queue bubbles; sampling keeps a live measurement inside a timed region without paying that per frame. */
int fs_set_profiling_interval(fs_context* ctx, int32_t frames);
int fs_get_stats(fs_context* ctx, fs_stats* out);
int fs_reset_stats(fs_context* ctx);
/* What the producer's side of a stream of frames did since the context was created (host counters, no device access, any time):
 * where a timed region can lose time that is not kernel time.  In the steady state of a single-GPU stream of pipelined frames
 * tail_stream_ops, stream_waits_enqueued and publishes_by_event stay constant: every launch goes onto the compute stream and
 * publishes its impulse responses by itself (the reference's contract: the IR is in the component's buffer when
 * ReconstructImpulseResponse returns, FSAC.cpp:377-378 — here: when the launch's id appears in a pinned host word). */
typedef struct fs_pipeline_counters {
    uint32_t struct_size;            /* = sizeof(fs_pipeline_counters), set by the caller */
    uint32_t reserved;
    uint64_t fused_launches;         /* launches that carry parts of several pipelined frames */
    uint64_t flushes, flushed_frames;/* held frames that had to finish on kernels of their own (fs_submit, fs_synchronize, an observer) */
    uint64_t host_waits, host_wait_us;   /* the producer waited for a publish: the IR ring's back-pressure, its only throttle */
    uint64_t stream_waits_enqueued;  /* waits for another stream's event put on the compute stream ... */
    uint64_t stream_waits_skipped;   /* ... and those not needed because the event had completed */
    uint64_t tail_stream_ops;        /* commands enqueued on the tail stream: hand-overs, reconstruct kernels, copies, event records, collectives */
    uint64_t owed_on_tail;           /* reconstructs that missed their fused launch and ran on kernels of their own */
    uint64_t publishes_by_word;      /* impulse responses published by the launch itself (compute stream, pinned host word) */
    uint64_t publishes_by_event;     /* ... through an event on the tail stream (a copy command or a batch kernel there) */
    uint64_t lane_launches;          /* first-stage launches of waited-for uncapped frames that carried a long-walk lane (cooperative waves for the longest walks) */
} fs_pipeline_counters;
int fs_get_pipeline_counters(fs_context* ctx, fs_pipeline_counters* out);
/* The context's HIP streams as hipStream_t values: the compute stream (fs_config.stream if the caller gave one, else the
 * context's own) and the tail stream (what fs_energy_handoff returns too).  For measurement — events recorded on the stream
 * the launches really go to — and for hosts that order work of their own behind a frame.  Either pointer may be NULL. */
int fs_get_streams(fs_context* ctx, void** compute_stream, void** tail_stream);

#if defined(FS_BUILDING_LIBRARY) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FREQUENSEE_H */
