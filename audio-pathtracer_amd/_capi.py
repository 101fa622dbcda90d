"""ctypes binding of include/frequensee.h (libfrequensee.so, HIP/gfx950).

There is no fallback: if the shared library is missing or a HIP device is unavailable every compute
call raises.  The product never imports oracle/.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfrequensee.so")

MAX_BANDS = 8
NO_MATERIAL = 0xFFFF
MAX_DEPTH = 64

OK = 0
ERR_INVALID_ARGUMENT = 1
ERR_NO_DEVICE = 2
ERR_HIP = 3
ERR_NOT_COMMITTED = 4
ERR_BAD_HANDLE = 5
ERR_SIZE_MISMATCH = 6
ERR_OUT_OF_MEMORY = 7

FLAG_FIXED_NORM_1000 = 1
FLAG_FLUSH_BEFORE_RECONSTRUCT = 2
FLAG_COSINE_SAMPLING = 4
FLAG_DETERMINISTIC = 8
FLAG_ALL_CONNECTIONS = 16
FLAG_MIS_BALANCE = 32
FLAG_MATERIAL_LOBES = 64
FLAG_ACCUMULATE_ENERGY = 128
FLAG_DOUBLE_POSITIONS = 256
FLAG_SPECTRAL_IR = 512   # reconstruct calls: the channel view as per-band noise carriers x band envelopes (include/frequensee.h)
FLAG_ROOM_PARAMETERS = 1024   # reconstruct calls: also publish each band's room parameters (fs_get_room_parameters)
NO_OBJECT = 0xFFFFFFFF

# every symbol include/frequensee.h declares (tests check the library exports all of them)
EXPORTS = [
    "fs_config_default", "fs_params_default", "fs_abi_version", "fs_context_create", "fs_context_destroy",
    "fs_last_error", "fs_context_advice", "fs_scene_set_triangles", "fs_scene_set_materials", "fs_scene_commit", "fs_source_create",
    "fs_source_destroy", "fs_source_set_position", "fs_listener_set_position", "fs_source_set_object", "fs_listener_set_object", "fs_compute_energy_response",
    "fs_compute_energy_response_async", "fs_compute_energy_response_batch_async", "fs_energy_device_ptr", "fs_reconstruct_impulse_response",
    "fs_reconstruct_impulse_response_async", "fs_reconstruct_impulse_response_batch_async", "fs_update_sources", "fs_synchronize", "fs_get_impulse_response", "fs_get_impulse_response_sequence",
    "fs_copy_impulse_response", "fs_copy_band_impulse_response", "fs_get_energy_buffer", "fs_flush_energy_buffer",
    "fs_add_energy_at_delay", "fs_update_energy_buffer", "fs_num_bins", "fs_num_samples", "fs_trace_rays",
    "fs_set_profiling", "fs_set_profiling_interval", "fs_get_stats", "fs_reset_stats", "fs_get_pipeline_counters", "fs_get_streams",
    "fs_sound_params_default", "fs_scene_set_objects", "fs_update_sound", "fs_get_occlusion_attenuation",
    "fs_save_array_to_file", "fs_load_float_array", "fs_save_impulse_response",
    "fs_reverb_init", "fs_reverb_process", "fs_reverb_process_batch", "fs_reverb_release", "fs_reverb_set_crossfade", "fs_reverb_set_engine",
    "fs_reverb_ears_default", "fs_reverb_ears_set", "fs_reverb_ears_info", "fs_reverb_set_ears", "fs_reverb_copy_ear_impulse_responses",
    "fs_reverb_soundfield_set", "fs_reverb_soundfield_info", "fs_reverb_set_soundfield", "fs_reverb_copy_soundfield_impulse_responses",
    "fs_reverb_soundfield_process_batch",
    "fs_apply_material_fd", "fs_energy_handoff", "fs_scene_update_triangles", "fs_scene_refit", "fs_scene_set_object_transforms", "fs_set_impulse_response",
    "fs_scene_commit_fast", "fs_comm_unique_id", "fs_comm_init", "fs_comm_attach", "fs_comm_detach", "fs_comm_info", "fs_comm_enable_oneshot", "fs_shard_range",
    "fs_peers_init", "fs_peers_detach", "fs_gather_energy", "fs_gather_energy_async", "fs_set_pipelining", "fs_set_walk_stages", "fs_set_frames_per_launch", "fs_submit", "fs_scene_commit_progressive", "fs_scene_refine_pending", "fs_scene_refine_wait",
    "fs_set_band_edges", "fs_source_set_orientation", "fs_source_set_directivity", "fs_get_room_parameters",
    "fs_source_set_order_window", "fs_source_get_order_window",
    "fs_direct_params_default", "fs_direct_sample_offsets", "fs_update_direct_paths",
    "fs_reflection_params_default", "fs_update_reflection_paths",
    "fs_diffraction_params_default", "fs_update_diffraction_paths",
    "fs_reflection2_params_default", "fs_update_reflection2_paths",
    "fs_diffraction2_params_default", "fs_update_diffraction2_paths",
    "fs_mixed_params_default", "fs_update_mixed_paths",
    "fs_pathing_set_probes", "fs_pathing_bake_params_default", "fs_pathing_bake", "fs_pathing_info", "fs_pathing_copy_graph",
    "fs_pathing_params_default", "fs_update_pathing_paths",
    "fs_direct_band_kernels", "fs_direct_render_init", "fs_direct_render_release", "fs_direct_render_process_batch",
    "fs_reflection_render_init", "fs_reflection_render_release", "fs_reflection_render_process_batch",
    "fs_hrtf_set", "fs_hrtf_info", "fs_hrtf_spherical_head",
    "fs_hrtf_triangulate", "fs_hrtf_mesh_rows", "fs_hrtf_mesh_locate", "fs_hrtf_set_mesh", "fs_hrtf_mesh_info",
    "fs_hrtf_set_onsets", "fs_hrtf_onsets_info", "fs_hrtf_delay", "fs_hrtf_split_onsets", "fs_hrtf_spherical_head_split",
    "fs_binaural_render_init", "fs_binaural_render_release", "fs_binaural_render_process_batch",
    "fs_ambisonic_encode", "fs_ambisonic_render_init", "fs_ambisonic_render_release", "fs_ambisonic_render_process_batch",
]
MAX_DIRECTIVITY_SAMPLES = 181   # FS_MAX_DIRECTIVITY_SAMPLES: 1 degree steps
ORDER_UNBOUNDED = 0x7fffffff    # FS_ORDER_UNBOUNDED: no upper end of a source's order window
COMM_ID_BYTES = 128
ERR_COMM = 8
ERR_OVERFLOW = 9
REVERB_LITERAL_TAIL = 1
MAX_REVERB_BATCH = 256
REVERB_ENGINE_DIRECT = 0
REVERB_ENGINE_PARTITIONED = 1
MAX_DIRECT_BATCH = 256
MAX_DIRECT_SAMPLES = 64
DIRECT_MAX_QUERIES = 32
MAX_DIRECT_RENDER_BATCH = 256
MAX_REFLECTIONS = 16
MAX_REFLECTION_CANDIDATES = 256
MAX_REFLECTION_BATCH = 256
REFLECTION_OVERFLOW = 1
MAX_DIFFRACTIONS = 16
MAX_DIFFRACTION_CANDIDATES = 2048
MAX_DIFFRACTION_BATCH = 256
DIFFRACTION_OVERFLOW = 1
DIFFRACTION_VOICE_TAG = 0x80000000   # the top bit of a diffraction voice's key: 0x80000000 | (4 triangle + edge)
MAX_REFLECTION2_PATHS = 32
MAX_REFLECTION2_NEAR = 32768
MAX_REFLECTION2_CANDIDATES = 1024
MAX_REFLECTION2_BATCH = 256
REFLECTION2_OVERFLOW = 1
REFLECTION2_NEAR_OVERFLOW = 2
REFLECTION2_VOICE_TAG = 0x40000000   # a second-order voice's key: 0x40000000 | (((a * 2654435761 + b) mod 2^32) >> 2)
MAX_DIFFRACTION2_PATHS = 16
MAX_DIFFRACTION2_NEAR = 32768
MAX_DIFFRACTION2_CANDIDATES = 2048
MAX_DIFFRACTION2_BATCH = 256
DIFFRACTION2_OVERFLOW = 1
DIFFRACTION2_NEAR_OVERFLOW = 2
DIFFRACTION2_VOICE_TAG = 0x20000000   # a second-order diffraction voice's key: 0x20000000 | (((kp * 2654435761 + kq) mod 2^32) >> 3), k = 4 triangle + edge
MAX_MIXED_PATHS = 16
MAX_MIXED_NEAR = 32768
MAX_MIXED_CANDIDATES = 2048
MAX_MIXED_BATCH = 256
MIXED_OVERFLOW = 1
MIXED_NEAR_OVERFLOW = 2
MIXED_VOICE_TAG = 0xC0000000   # a mixed voice's key: 0xC0000000 | (((m * 2654435761 + 4 (2 (4 i + j) + end)) mod 2^32) >> 2)
MAX_PATHING_PROBES = 1024
MAX_PATHING_NODES = 16
MAX_PATHING_BATCH = 256
PATHING_MIN_EDGE = 1.0
PATHING_MAX_LENGTH = 1048576.0
PATHING_FOUND = 1
PATHING_DIRECT = 2
PATHING_STALE = 4
PATHING_NO_PROBE = 0xFFFFFFFF
PATHING_VOICE_KEY = 0x80000003   # a pathing voice's key: a first-order diffraction key 0x80000000 | (4 triangle + edge) never ends in binary 11
DIRECT_RENDER_MAX_TAPS = 2047
MAX_REFLECTION_VOICES = 32
MAX_REFLECTION_RENDER_BATCH = 256
MAX_HRTF_DIRECTIONS = 4096
MAX_HRTF_TAPS = 512
HRTF_DEFAULT_RADIUS_CM = 8.75
HRTF_DEFAULT_SOUND_SPEED_CM_S = 34300.0
MAX_AMBISONIC_ORDER = 3   # FS_MAX_AMBISONIC_ORDER: the bus has (order + 1)^2 channels, ACN order, SN3D normalisation
BINAURAL_DIRECT_KEY = 0x1FFFFFFF   # the direct sound's voice: a first-order key (a triangle index) no scene below 2^29 - 1 triangles uses


class SoundParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("raycasts_per_tick", C.c_int32),
        ("seed", C.c_uint64),
        ("raycast_bounces", C.c_int32),
        ("raycast_distance", C.c_float),
        ("simulated_duration", C.c_float),
        ("listener_radius", C.c_float),
    ]


class SoundResult(C.Structure):
    _fields_ = [
        ("total_energy", C.c_float),
        ("occlusion_attenuation", C.c_float),
        ("direct_energy_sum", C.c_float),
        ("rays_reaching_listener", C.c_uint32),
        ("direct_hits", C.c_uint32),
        ("traces", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("num_bands", C.c_int32),
        ("sample_rate", C.c_int32),
        ("num_channels", C.c_int32),
        ("simulated_duration", C.c_float),
        ("bin_duration", C.c_float),
        ("rank", C.c_int32),
        ("world_size", C.c_int32),
        ("stream", C.c_void_p),
    ]


class Params(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("flags", C.c_uint32),
        ("seed", C.c_uint64),
        ("num_rays", C.c_uint32),
        ("depth", C.c_int32),
        ("russian_roulette", C.c_int32),
        ("rr_prob", C.c_float),
        ("max_trace_dist", C.c_float),
        ("surface_offset", C.c_float),
        ("connect_pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("min_seg", C.c_float),
        ("prob_exponent", C.c_float),
        ("energy_clamp", C.c_float),
        ("energy_gain", C.c_float),
        ("sound_speed", C.c_float),
        ("air_absorption", C.c_float * MAX_BANDS),
        ("samples_per_bin", C.c_int32),
        ("listener_radius", C.c_float),
        ("source_radius", C.c_float),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("frames", C.c_uint64),
        ("rays", C.c_uint64),
        ("pairs", C.c_uint64),
        ("walk_kernel_ms_sum", C.c_double),
        ("walk_kernel_ms_last", C.c_double),
        ("connect_kernel_ms_sum", C.c_double),
        ("reconstruct_ms_sum", C.c_double),
        ("timed_frames", C.c_uint64),
        ("timed_connects", C.c_uint64),
        ("timed_reconstructs", C.c_uint64),
        ("bvh_nodes", C.c_uint32),
        ("triangles", C.c_uint32),
        ("bvh_stack_need", C.c_uint32),
        ("bvh_depth", C.c_uint32),
        ("scene_bytes", C.c_uint64),
        ("segments", C.c_uint64),
        ("connections_tested", C.c_uint64),
        ("deposits", C.c_uint64),
        ("walk_node_fetches", C.c_uint64),
        ("walk_tri_fetches", C.c_uint64),
        ("any_node_fetches", C.c_uint64),
        ("any_tri_fetches", C.c_uint64),
        ("node_request_insts", C.c_uint64),
        ("node_request_lanes", C.c_uint64),
        ("node_request_distinct", C.c_uint64),
        ("planned_segments", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PipelineCounters(C.Structure):
    """fs_pipeline_counters (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("fused_launches", C.c_uint64),
        ("flushes", C.c_uint64),
        ("flushed_frames", C.c_uint64),
        ("host_waits", C.c_uint64),
        ("host_wait_us", C.c_uint64),
        ("stream_waits_enqueued", C.c_uint64),
        ("stream_waits_skipped", C.c_uint64),
        ("tail_stream_ops", C.c_uint64),
        ("owed_on_tail", C.c_uint64),
        ("publishes_by_word", C.c_uint64),
        ("publishes_by_event", C.c_uint64),
        ("lane_launches", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k not in ("struct_size", "reserved")}


class RoomParameters(C.Structure):
    """fs_room_parameters (include/frequensee.h): one band's record, an array element (no struct_size)"""
    _fields_ = [(k, C.c_float) for k in ("energy", "onset", "edt", "t20", "t30", "c50", "c80", "d50", "ts")]


class DirectParams(C.Structure):
    """fs_direct_params (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("samples", C.c_int32),
        ("source_radius", C.c_float),
        ("max_surfaces", C.c_int32),
        ("step", C.c_float),
        ("pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("sound_speed", C.c_float),
    ]


class DirectPath(C.Structure):
    """fs_direct_path (include/frequensee.h): one source's row, an array element (no struct_size)"""
    _fields_ = [
        ("distance", C.c_float),
        ("delay", C.c_float),
        ("visibility", C.c_float),
        ("surfaces", C.c_uint32),
        ("samples_valid", C.c_uint32),
        ("transmission", C.c_float * MAX_BANDS),
    ]


class ReflectionParams(C.Structure):
    """fs_reflection_params (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_paths", C.c_int32),
        ("max_candidates", C.c_int32),
        ("margin", C.c_float),
        ("step", C.c_float),
        ("offset", C.c_float),
        ("pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("sound_speed", C.c_float),
    ]


class ReflectionPath(C.Structure):
    """fs_reflection_path (include/frequensee.h): one reflection of one source, an array element (no struct_size)"""
    _fields_ = [
        ("length", C.c_float),
        ("delay", C.c_float),
        ("point", C.c_float * 3),
        ("direction", C.c_float * 3),
        ("triangle", C.c_uint32),
        ("material", C.c_uint32),
        ("reflectance", C.c_float * MAX_BANDS),
    ]


class ReflectionRow(C.Structure):
    """fs_reflection_row (include/frequensee.h): one source's counts, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("candidates", "found", "returned", "flags")]


class DiffractionParams(C.Structure):
    """fs_diffraction_params (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_paths", C.c_int32),
        ("max_candidates", C.c_int32),
        ("margin", C.c_float),
        ("max_detour", C.c_float),
        ("offset", C.c_float),
        ("merge", C.c_float),
        ("step", C.c_float),
        ("pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("sound_speed", C.c_float),
    ]


class DiffractionPath(C.Structure):
    """fs_diffraction_path (include/frequensee.h): one diffraction path of one source, an array element (no struct_size)"""
    _fields_ = [
        ("length", C.c_float),
        ("delay", C.c_float),
        ("detour", C.c_float),
        ("cos_bend", C.c_float),
        ("apex", C.c_float * 3),
        ("direction", C.c_float * 3),
        ("triangle", C.c_uint32),
        ("edge", C.c_uint32),
        ("material", C.c_uint32),
        ("gain", C.c_float * MAX_BANDS),
    ]


class DiffractionRow(C.Structure):
    """fs_diffraction_row (include/frequensee.h): one source's counts, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("candidates", "confirmed", "found", "returned", "flags")]


class Reflection2Params(C.Structure):
    """fs_reflection2_params (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_paths", C.c_int32),
        ("max_near", C.c_int32),
        ("max_candidates", C.c_int32),
        ("max_length", C.c_float),
        ("margin", C.c_float),
        ("step", C.c_float),
        ("offset", C.c_float),
        ("pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("sound_speed", C.c_float),
    ]


class Reflection2Path(C.Structure):
    """fs_reflection2_path (include/frequensee.h): one second-order reflection of one source, an array element (no struct_size)"""
    _fields_ = [
        ("length", C.c_float),
        ("delay", C.c_float),
        ("point", (C.c_float * 3) * 2),
        ("direction", C.c_float * 3),
        ("triangle", C.c_uint32 * 2),
        ("material", C.c_uint32 * 2),
        ("reflectance", C.c_float * MAX_BANDS),
    ]


class Reflection2Row(C.Structure):
    """fs_reflection2_row (include/frequensee.h): one source's counts, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("near", "candidates", "found", "returned", "flags")]


class Diffraction2Params(C.Structure):
    """fs_diffraction2_params (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_paths", C.c_int32),
        ("max_near", C.c_int32),
        ("max_candidates", C.c_int32),
        ("margin", C.c_float),
        ("max_detour", C.c_float),
        ("min_parallel", C.c_float),
        ("offset", C.c_float),
        ("merge", C.c_float),
        ("step", C.c_float),
        ("pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("sound_speed", C.c_float),
    ]


class Diffraction2Path(C.Structure):
    """fs_diffraction2_path (include/frequensee.h): one path round two edges of one source, an array element (no struct_size)"""
    _fields_ = [
        ("length", C.c_float),
        ("delay", C.c_float),
        ("detour", C.c_float),
        ("gap", C.c_float),
        ("cos_bend", C.c_float * 2),
        ("apex", (C.c_float * 3) * 2),
        ("direction", C.c_float * 3),
        ("triangle", C.c_uint32 * 2),
        ("edge", C.c_uint32 * 2),
        ("material", C.c_uint32 * 2),
        ("gain", C.c_float * MAX_BANDS),
    ]


class Diffraction2Row(C.Structure):
    """fs_diffraction2_row (include/frequensee.h): one source's counts, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("near", "candidates", "confirmed", "found", "returned", "flags")]


class MixedParams(C.Structure):
    """fs_mixed_params (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_paths", C.c_int32),
        ("max_near", C.c_int32),
        ("max_candidates", C.c_int32),
        ("max_length", C.c_float),
        ("max_detour", C.c_float),
        ("margin", C.c_float),
        ("offset", C.c_float),
        ("merge", C.c_float),
        ("step", C.c_float),
        ("pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("sound_speed", C.c_float),
    ]


class MixedPath(C.Structure):
    """fs_mixed_path (include/frequensee.h): one path off a reflector and round an edge of one source, an array element (no struct_size)"""
    _fields_ = [
        ("length", C.c_float),
        ("delay", C.c_float),
        ("detour", C.c_float),
        ("bend_detour", C.c_float),
        ("cos_bend", C.c_float),
        ("apex", C.c_float * 3),
        ("point", C.c_float * 3),
        ("direction", C.c_float * 3),
        ("end", C.c_uint32),
        ("triangle", C.c_uint32 * 2),
        ("edge", C.c_uint32),
        ("material", C.c_uint32 * 2),
        ("gain", C.c_float * MAX_BANDS),
    ]


class MixedRow(C.Structure):
    """fs_mixed_row (include/frequensee.h): one source's counts, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("near", "candidates", "confirmed", "found", "returned", "flags")]


class PathingBakeParams(C.Structure):
    """fs_pathing_bake_params (include/frequensee.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("max_edge", C.c_float), ("step", C.c_float)]


class PathingParams(C.Structure):
    """fs_pathing_params (include/frequensee.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("validate", C.c_int32),
        ("max_attach", C.c_float),
        ("max_length", C.c_float),
        ("step", C.c_float),
        ("pullback", C.c_float),
        ("dist_divisor", C.c_float),
        ("sound_speed", C.c_float),
    ]


class PathingPath(C.Structure):
    """fs_pathing_path (include/frequensee.h): one source's route through the probe graph, an array element (no struct_size)"""
    _fields_ = [
        ("length", C.c_float),
        ("delay", C.c_float),
        ("detour", C.c_float),
        ("distance", C.c_float),
        ("direction", C.c_float * 3),
        ("departure", C.c_float * 3),
        ("hops", C.c_uint32),
        ("flags", C.c_uint32),
        ("first_probe", C.c_uint32),
        ("last_probe", C.c_uint32),
        ("probes", C.c_uint32 * MAX_PATHING_NODES),
        ("gain", C.c_float * MAX_BANDS),
    ]


class DirectRenderTarget(C.Structure):
    """fs_direct_render_target (include/frequensee.h): one source's target of a callback, an array element (no struct_size)"""
    _fields_ = [
        ("delay", C.c_float),
        ("band_gain", C.c_float * MAX_BANDS),
    ]


class ReflectionVoice(C.Structure):
    """fs_reflection_voice (include/frequensee.h): one entry of a source's voice list, an array element (no struct_size)"""
    _fields_ = [
        ("key", C.c_uint32),
        ("delay", C.c_float),
        ("band_gain", C.c_float * MAX_BANDS),
        ("channel_gain", C.c_float * 2),
    ]


class ReflectionRenderRow(C.Structure):
    """fs_reflection_render_row (include/frequensee.h): one source's counts of a callback, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("sounding", "started", "ended", "dropped")]


class HrtfDesc(C.Structure):
    """fs_hrtf_desc (include/frequensee.h): the HRIR set handed to fs_hrtf_set"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("directions", C.c_int32),
        ("taps", C.c_int32),
        ("sample_rate", C.c_int32),
        ("dirs", C.c_void_p),
        ("hrir", C.c_void_p),
    ]


class ReverbEarsDesc(C.Structure):
    """fs_reverb_ears_desc (include/frequensee.h): the head of fs_reverb_ears_set's diffuse-field coherence"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("radius_cm", C.c_float),
        ("sound_speed_cm_s", C.c_float),
    ]


class BinauralVoice(C.Structure):
    """fs_binaural_voice (include/frequensee.h): one entry of a source's voice list, an array element (no struct_size)"""
    _fields_ = [
        ("key", C.c_uint32),
        ("delay", C.c_float),
        ("band_gain", C.c_float * MAX_BANDS),
        ("gain", C.c_float),
        ("direction", C.c_float * 3),
    ]


class BinauralRenderRow(C.Structure):
    """fs_binaural_render_row (include/frequensee.h): one source's counts of a callback, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("sounding", "started", "ended", "dropped")]


AmbisonicVoice = BinauralVoice   # fs_ambisonic_voice: the same record


class AmbisonicRenderRow(C.Structure):
    """fs_ambisonic_render_row (include/frequensee.h): one source's counts of a callback, an array element (no struct_size)"""
    _fields_ = [(k, C.c_uint32) for k in ("sounding", "started", "ended", "dropped")]


# one path query of include/frequensee.h; row None: an out-only query, one path record per source and no counts
PathQuery = collections.namedtuple("PathQuery", "kind params row path max_batch default update")


def _path_query(kind, params, row, path, max_batch):
    return PathQuery(kind, params, row, path, max_batch, f"fs_{kind}_params_default", f"fs_update_{kind}_paths")


# The path queries, in the order they were added.  What is the same for all of them — the binding's signatures and defaults
# (below), Context's and AudioRayTracingSubsystem's methods (component.py), the tests' contract (tests/path_query_contract.py)
# — is written once and reads its row here.
PATH_QUERIES = (
    _path_query("direct", DirectParams, None, DirectPath, MAX_DIRECT_BATCH),
    _path_query("reflection", ReflectionParams, ReflectionRow, ReflectionPath, MAX_REFLECTION_BATCH),
    _path_query("diffraction", DiffractionParams, DiffractionRow, DiffractionPath, MAX_DIFFRACTION_BATCH),
    _path_query("reflection2", Reflection2Params, Reflection2Row, Reflection2Path, MAX_REFLECTION2_BATCH),
    _path_query("diffraction2", Diffraction2Params, Diffraction2Row, Diffraction2Path, MAX_DIFFRACTION2_BATCH),
    _path_query("mixed", MixedParams, MixedRow, MixedPath, MAX_MIXED_BATCH),
    _path_query("pathing", PathingParams, None, PathingPath, MAX_PATHING_BATCH),
)
PATH_QUERY = {q.kind: q for q in PATH_QUERIES}


@functools.lru_cache(maxsize=None)
def record_dtype(struct):
    """the numpy dtype of a ctypes structure: the same field names, offsets and itemsize; an array of arrays such as
    (c_float * 3) * 2 is one field of shape (2, 3)"""
    import numpy as np
    names, formats, offsets = [], [], []
    for name, ctype in struct._fields_:
        shape = ()
        while hasattr(ctype, "_length_"):
            shape, ctype = shape + (ctype._length_,), ctype._type_
        names.append(name)
        formats.append((np.dtype(ctype), shape))
        offsets.append(getattr(struct, name).offset)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=C.sizeof(struct)))


class FrequenSeeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"frequensee status {code}: {msg}")
        self.code = code


_lib = None


def load():
    """Load libfrequensee.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # Host requirement of the library (fs_context_advice): 16 hardware queues, decided before the
    # HIP runtime initialises — this binding is the host here.  An explicit setting of the process wins.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    lib = C.CDLL(LIB_PATH)
    vp, i32, u16p, f32p = C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p
    sig = {
        "fs_config_default": (None, [C.POINTER(Config)]),
        "fs_params_default": (None, [C.POINTER(Params)]),
        "fs_abi_version": (C.c_int, []),
        "fs_context_create": (C.c_int, [C.POINTER(Config), C.POINTER(vp)]),
        "fs_context_destroy": (C.c_int, [vp]),
        "fs_last_error": (C.c_char_p, [vp]),
        "fs_context_advice": (C.c_char_p, [vp]),
        "fs_scene_set_triangles": (C.c_int, [vp, f32p, u16p, i32]),
        "fs_scene_set_materials": (C.c_int, [vp, f32p, f32p, f32p, i32, i32]),
        "fs_scene_commit": (C.c_int, [vp]),
        "fs_scene_commit_fast": (C.c_int, [vp]),
        "fs_source_create": (C.c_int, [vp, C.POINTER(i32)]),
        "fs_source_destroy": (C.c_int, [vp, i32]),
        "fs_source_set_position": (C.c_int, [vp, i32, C.POINTER(C.c_float)]),
        "fs_listener_set_position": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "fs_source_set_object": (C.c_int, [vp, i32, C.c_uint32]),
        "fs_listener_set_object": (C.c_int, [vp, C.c_uint32]),
        "fs_source_set_orientation": (C.c_int, [vp, i32, C.POINTER(C.c_float)]),
        "fs_source_set_directivity": (C.c_int, [vp, i32, f32p, i32, i32]),
        "fs_source_set_order_window": (C.c_int, [vp, i32, i32, i32]),
        "fs_source_get_order_window": (C.c_int, [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fs_compute_energy_response": (C.c_int, [vp, i32, C.POINTER(Params), f32p]),
        "fs_compute_energy_response_async": (C.c_int, [vp, i32, C.POINTER(Params)]),
        "fs_compute_energy_response_batch_async": (C.c_int, [vp, C.POINTER(C.c_int32), i32, C.POINTER(Params)]),
        "fs_energy_device_ptr": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "fs_scene_update_triangles": (C.c_int, [vp, i32, i32, f32p]),
        "fs_scene_refit": (C.c_int, [vp]),
        "fs_scene_set_object_transforms": (C.c_int, [vp, C.c_void_p, f32p, i32]),
        "fs_set_impulse_response": (C.c_int, [vp, i32, f32p, i32]),
        "fs_energy_handoff": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]),
        "fs_reconstruct_impulse_response": (C.c_int, [vp, i32, C.POINTER(Params)]),
        "fs_reconstruct_impulse_response_async": (C.c_int, [vp, i32, C.POINTER(Params)]),
        "fs_reconstruct_impulse_response_batch_async": (C.c_int, [vp, C.POINTER(C.c_int32), i32, C.POINTER(Params)]),
        "fs_update_sources": (C.c_int, [vp, C.POINTER(C.c_int32), i32, C.POINTER(Params)]),
        "fs_synchronize": (C.c_int, [vp]),
        "fs_get_impulse_response": (C.c_int, [vp, i32, i32, C.POINTER(C.POINTER(C.c_float)), C.POINTER(i32)]),
        "fs_copy_impulse_response": (C.c_int, [vp, i32, i32, f32p, i32]),
        "fs_get_impulse_response_sequence": (C.c_int, [vp, i32, C.POINTER(C.c_uint64)]),
        "fs_get_room_parameters": (C.c_int, [vp, i32, C.POINTER(RoomParameters), i32, C.POINTER(C.c_uint64)]),
        "fs_copy_band_impulse_response": (C.c_int, [vp, i32, i32, f32p, i32]),
        "fs_get_energy_buffer": (C.c_int, [vp, i32, f32p, i32]),
        "fs_flush_energy_buffer": (C.c_int, [vp, i32]),
        "fs_add_energy_at_delay": (C.c_int, [vp, i32, i32, C.c_float, C.c_float]),
        "fs_update_energy_buffer": (C.c_int, [vp, i32, f32p, i32]),
        "fs_num_bins": (C.c_int, [vp]),
        "fs_num_samples": (C.c_int, [vp]),
        "fs_trace_rays": (C.c_int, [vp, f32p, f32p, f32p, i32, i32, vp, f32p, vp, f32p]),
        "fs_set_profiling": (C.c_int, [vp, i32]),
        "fs_set_profiling_interval": (C.c_int, [vp, i32]),
        "fs_get_stats": (C.c_int, [vp, C.POINTER(Stats)]),
        "fs_reset_stats": (C.c_int, [vp]),
        "fs_get_pipeline_counters": (C.c_int, [vp, C.POINTER(PipelineCounters)]),
        "fs_get_streams": (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
        "fs_sound_params_default": (None, [C.POINTER(SoundParams)]),
        "fs_scene_set_objects": (C.c_int, [vp, vp, i32]),
        "fs_update_sound": (C.c_int, [vp, i32, C.POINTER(SoundParams), C.POINTER(SoundResult)]),
        "fs_get_occlusion_attenuation": (C.c_int, [vp, i32, C.POINTER(C.c_float)]),
        "fs_save_array_to_file": (C.c_int, [f32p, i32, C.c_char_p]),
        "fs_load_float_array": (C.c_int, [C.c_char_p, f32p, i32, C.POINTER(i32)]),
        "fs_save_impulse_response": (C.c_int, [vp, i32, i32, C.c_char_p]),
        "fs_reverb_init": (C.c_int, [vp, i32, i32]),
        "fs_reverb_process": (C.c_int, [vp, i32, f32p, f32p, i32, C.c_uint32]),
        "fs_reverb_process_batch": (C.c_int, [vp, C.c_void_p, i32, f32p, f32p, C.c_void_p, C.c_uint32, f32p]),
        "fs_reverb_release": (C.c_int, [vp, i32]),
        "fs_reverb_set_crossfade": (C.c_int, [vp, i32, i32]),
        "fs_reverb_set_engine": (C.c_int, [vp, i32, i32]),
        "fs_reverb_ears_default": (None, [C.POINTER(ReverbEarsDesc)]),
        "fs_reverb_ears_set": (C.c_int, [vp, C.POINTER(ReverbEarsDesc)]),
        "fs_reverb_ears_info": (C.c_int, [vp, f32p, f32p, C.c_void_p]),
        "fs_reverb_set_ears": (C.c_int, [vp, i32, i32]),
        "fs_reverb_copy_ear_impulse_responses": (C.c_int, [vp, i32, f32p, f32p, i32]),
        "fs_reverb_soundfield_set": (C.c_int, [vp, i32]),
        "fs_reverb_soundfield_info": (C.c_int, [vp, C.c_void_p, C.c_void_p]),
        "fs_reverb_set_soundfield": (C.c_int, [vp, i32, i32]),
        "fs_reverb_copy_soundfield_impulse_responses": (C.c_int, [vp, i32, f32p, i32]),
        "fs_reverb_soundfield_process_batch": (C.c_int, [vp, C.c_void_p, i32, f32p, C.c_void_p, C.c_uint32, C.c_void_p]),
        "fs_apply_material_fd": (C.c_int, [vp, f32p, i32, f32p, f32p, f32p, i32, f32p, f32p, f32p]),
        "fs_comm_unique_id": (C.c_int, [vp, C.c_size_t]),
        "fs_comm_init": (C.c_int, [vp, vp, C.c_size_t]),
        "fs_comm_attach": (C.c_int, [vp, vp]),
        "fs_comm_detach": (C.c_int, [vp]),
        "fs_comm_info": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fs_comm_enable_oneshot": (C.c_int, [vp]),
        "fs_shard_range": (C.c_int, [C.c_uint32, i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "fs_peers_init": (C.c_int, [vp, vp, C.c_size_t, i32, i32]),
        "fs_peers_detach": (C.c_int, [vp]),
        "fs_set_pipelining": (C.c_int, [vp, i32]),
        "fs_set_walk_stages": (C.c_int, [vp, vp, i32]),
        "fs_set_frames_per_launch": (C.c_int, [vp, i32]),
        "fs_set_band_edges": (C.c_int, [vp, vp, i32]),
        "fs_submit": (C.c_int, [vp]),
        "fs_scene_commit_progressive": (C.c_int, [vp]),
        "fs_scene_refine_pending": (C.c_int, [vp, C.POINTER(i32)]),
        "fs_scene_refine_wait": (C.c_int, [vp]),
        "fs_direct_sample_offsets": (C.c_int, [i32, f32p]),
        "fs_pathing_set_probes": (C.c_int, [vp, C.c_void_p, i32]),
        "fs_pathing_bake_params_default": (None, [C.POINTER(PathingBakeParams)]),
        "fs_pathing_bake": (C.c_int, [vp, C.POINTER(PathingBakeParams)]),
        "fs_pathing_info": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fs_pathing_copy_graph": (C.c_int, [vp, C.c_void_p, i32]),
        "fs_direct_band_kernels": (C.c_int, [i32, f32p, i32, i32, f32p]),
        "fs_direct_render_init": (C.c_int, [vp, i32, i32, i32, C.c_float]),
        "fs_direct_render_release": (C.c_int, [vp, i32]),
        "fs_direct_render_process_batch": (C.c_int, [vp, C.c_void_p, i32, f32p, C.c_void_p, f32p, f32p]),
        "fs_reflection_render_init": (C.c_int, [vp, i32, i32, i32, i32, C.c_float]),
        "fs_reflection_render_release": (C.c_int, [vp, i32]),
        "fs_reflection_render_process_batch": (C.c_int, [vp, C.c_void_p, i32, f32p, C.c_void_p, C.c_void_p, i32, f32p, f32p, C.c_void_p]),
        "fs_hrtf_set": (C.c_int, [vp, C.POINTER(HrtfDesc)]),
        "fs_hrtf_info": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fs_hrtf_spherical_head": (C.c_int, [i32, C.c_float, C.c_float, i32, i32, f32p, f32p]),
        "fs_hrtf_triangulate": (C.c_int, [f32p, i32, C.c_void_p, i32, C.POINTER(C.c_int32)]),
        "fs_hrtf_mesh_rows": (C.c_int, [f32p, i32, C.c_void_p, i32, f32p]),
        "fs_hrtf_mesh_locate": (C.c_int, [f32p, i32, f32p, C.POINTER(C.c_int32), f32p]),
        "fs_hrtf_set_mesh": (C.c_int, [vp, C.c_void_p, i32]),
        "fs_hrtf_mesh_info": (C.c_int, [vp, C.POINTER(C.c_int32)]),
        "fs_hrtf_set_onsets": (C.c_int, [vp, f32p]),
        "fs_hrtf_onsets_info": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fs_hrtf_delay": (C.c_int, [f32p, i32, C.c_float, f32p, i32]),
        "fs_hrtf_split_onsets": (C.c_int, [f32p, i32, i32, C.c_float, i32, f32p, f32p]),
        "fs_hrtf_spherical_head_split": (C.c_int, [i32, C.c_float, C.c_float, i32, i32, f32p, f32p, f32p]),
        "fs_binaural_render_init": (C.c_int, [vp, i32, i32, i32, i32, C.c_float]),
        "fs_binaural_render_release": (C.c_int, [vp, i32]),
        "fs_binaural_render_process_batch": (C.c_int, [vp, C.c_void_p, i32, f32p, C.c_void_p, C.c_void_p, i32, f32p, f32p, C.c_void_p]),
        "fs_ambisonic_encode": (C.c_int, [i32, f32p, f32p]),
        "fs_ambisonic_render_init": (C.c_int, [vp, i32, i32, i32, i32, C.c_float, i32]),
        "fs_ambisonic_render_release": (C.c_int, [vp, i32]),
        "fs_ambisonic_render_process_batch": (C.c_int, [vp, C.c_void_p, i32, f32p, C.c_void_p, C.c_void_p, i32, f32p, f32p, C.c_void_p]),
        "fs_gather_energy": (C.c_int, [vp, i32, f32p, i32]),
        "fs_gather_energy_async": (C.c_int, [vp, i32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    }
    for q in PATH_QUERIES:   # fs_update_*_paths(ctx, sources, count, params, rows (not the out-only queries), paths)
        sig[q.default] = (None, [C.POINTER(q.params)])
        sig[q.update] = (C.c_int, [vp, C.c_void_p, i32, C.POINTER(q.params)] + [C.c_void_p] * (1 if q.row is None else 2))
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _defaults(struct, fill, kw):
    """a struct as the library's fs_*_default call fills it, then the caller's fields"""
    p = struct()
    getattr(load(), fill)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_config(**kw) -> Config:
    return _defaults(Config, "fs_config_default", kw)


def default_sound_params(**kw) -> SoundParams:
    return _defaults(SoundParams, "fs_sound_params_default", kw)


def default_reverb_ears(**kw) -> ReverbEarsDesc:
    return _defaults(ReverbEarsDesc, "fs_reverb_ears_default", kw)


def default_pathing_bake_params(**kw) -> PathingBakeParams:
    return _defaults(PathingBakeParams, "fs_pathing_bake_params_default", kw)


def default_path_params(kind, **kw):
    """the params of the path query `kind` (PATH_QUERY) as its fs_*_params_default fills them, then the caller's fields"""
    q = PATH_QUERY[kind]
    return _defaults(q.params, q.default, kw)


# default_<kind>_params(**kw), one per row of PATH_QUERIES in its order
(default_direct_params, default_reflection_params, default_diffraction_params, default_reflection2_params, default_diffraction2_params,
 default_mixed_params, default_pathing_params) = (functools.partial(default_path_params, q.kind) for q in PATH_QUERIES)


def default_params(**kw) -> Params:
    air = kw.pop("air_absorption", None)
    p = _defaults(Params, "fs_params_default", kw)
    if air is not None:
        for i, x in enumerate(air):
            p.air_absorption[i] = float(x)
    return p


def save_array_to_file(array, path):
    """SaveArrayToFile (FSAC.cpp:492-505): one SanitizeFloat'ed value per line"""
    import numpy as np
    a = np.ascontiguousarray(array, dtype=np.float32).reshape(-1)
    rc = load().fs_save_array_to_file(a.ctypes.data, a.shape[0], str(path).encode())
    if rc != OK:
        raise FrequenSeeError(rc, f"cannot write {path}")


def load_float_array(path):
    """LoadFloatArray (FSAC.cpp:454-490)"""
    import numpy as np
    n = C.c_int32()
    lib = load()
    rc = lib.fs_load_float_array(str(path).encode(), None, 0, C.byref(n))
    if rc != OK:
        raise FrequenSeeError(rc, f"cannot read {path}")
    out = np.zeros(n.value, dtype=np.float32)
    lib.fs_load_float_array(str(path).encode(), out.ctypes.data, out.shape[0], C.byref(n))
    return out
