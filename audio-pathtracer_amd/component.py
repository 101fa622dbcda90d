"""Host-side mirror of the reference's plugin interface for the BDPT path, over the C ABI.

  AudioRayTracingSubsystem  <->  UAudioRayTracingSubsystem   (Public/AudioRayTracingSubsystem.h:86-196)
  FrequenSeeAudioComponent  <->  UFrequenSeeAudioComponent   (Public/FrequenSeeAudioComponent.h:20-154)

Same method names, argument meaning and error behaviour (check() aborts become exceptions), so the
parity tests read like tests of the reference.  All compute happens in libfrequensee.so (HIP).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import FrequenSeeError, record_dtype


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


class Context:
    """Thin RAII wrapper of fs_context (one HIP device, one stream)."""

    def __init__(self, num_bands=1, device=0, rank=0, world_size=1, stream=None, **cfg):
        self.lib = _capi.load()
        c = _capi.default_config(num_bands=num_bands, device=device, rank=rank, world_size=world_size, **cfg)
        if stream is not None:
            c.stream = C.c_void_p(int(stream))
        self.cfg = c
        h = C.c_void_p()
        rc = self.lib.fs_context_create(C.byref(c), C.byref(h))
        self.h = h
        if rc != _capi.OK:
            msg = self.lib.fs_last_error(h).decode() if h else "fs_context_create failed"
            if h:
                self.lib.fs_context_destroy(h)
                self.h = None
            raise FrequenSeeError(rc, msg)
        self.num_bands = num_bands
        self.num_bins = self.lib.fs_num_bins(self.h)
        self.num_samples = self.lib.fs_num_samples(self.h)

    def check(self, rc):
        if rc != _capi.OK:
            raise FrequenSeeError(rc, self.lib.fs_last_error(self.h).decode())

    def advice(self):
        """fs_context_advice: what fs_context_create found worth telling the host about its environment ('' = nothing)"""
        return self.lib.fs_context_advice(self.h).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.fs_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- multi-GPU: the library's own RCCL communicator (include/frequensee.h) ----
    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: the 128-byte id every rank passes to comm_init (ship it with any host-side transport)"""
        buf = (C.c_char * _capi.COMM_ID_BYTES)()
        rc = _capi.load().fs_comm_unique_id(buf, _capi.COMM_ID_BYTES)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_comm_unique_id failed (librccl not loadable?)")
        return bytes(buf)

    def comm_init(self, unique_id: bytes):
        """collective over the world_size ranks: from now on every frame's energy buffer is summed over the ranks on
        the tail stream, and set_scene lets rank 0 build the acceleration structure for all"""
        if len(unique_id) != _capi.COMM_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        buf = (C.c_char * _capi.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self.check(self.lib.fs_comm_init(self.h, buf, _capi.COMM_ID_BYTES))

    def comm_attach(self, nccl_comm: int):
        self.check(self.lib.fs_comm_attach(self.h, C.c_void_p(int(nccl_comm))))

    def comm_enable_oneshot(self):
        """collective: the energy buffer's sum over the ranks as one peer-write exchange (HIP IPC mailboxes) instead of ncclAllReduce"""
        self.check(self.lib.fs_comm_enable_oneshot(self.h))

    def comm_info(self):
        """fs_comm_info: (ranks of the attached communicator as RCCL counts them, this rank, collective kind 0 / 1 / 2)"""
        n, r, k = C.c_int32(), C.c_int32(), C.c_int32()
        self.check(self.lib.fs_comm_info(self.h, C.byref(n), C.byref(r), C.byref(k)))
        return int(n.value), int(r.value), int(k.value)

    def comm_detach(self):
        self.check(self.lib.fs_comm_detach(self.h))

    # cfg5: independent sources, one per GPU — a peer communicator for the optional all-gather
    def peers_init(self, unique_id: bytes, rank: int, world_size: int):
        """collective over the processes that each own a source; frames are not sharded or reduced by it"""
        if len(unique_id) != _capi.COMM_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        buf = (C.c_char * _capi.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self.check(self.lib.fs_peers_init(self.h, buf, _capi.COMM_ID_BYTES, int(rank), int(world_size)))
        self._peers = int(world_size)

    def peers_detach(self):
        self.check(self.lib.fs_peers_detach(self.h))
        self._peers = 0

    def gather_energy(self, src: int) -> np.ndarray:
        """collective: [world_size][B][bins] — entry r is the current frame's histogram of the source rank r passed"""
        n = int(getattr(self, "_peers", 0))
        out = np.empty((max(n, 1), self.num_bands, self.num_bins), np.float32)
        self.check(self.lib.fs_gather_energy(self.h, int(src), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def set_pipelining(self, depth):
        """0 / False: off; 1 / True: a frame's connect pass is held back and launched with the next frame's walk; 2: its walk
        is held back as well — one launch plans frame f, walks f - 1 and connects f - 2 (include/frequensee.h)"""
        self.check(self.lib.fs_set_pipelining(self.h, int(depth)))

    def set_frames_per_launch(self, n: int):
        """fs_set_frames_per_launch: with pipelining on, plain frames wait until n have come and share one launch (every frame
        keeps its seed, energy buffer and recorded reconstruct: the results are those of n single frames)"""
        self.check(self.lib.fs_set_frames_per_launch(self.h, int(n)))

    def set_walk_stages(self, bounds):
        """fs_set_walk_stages: the steps at which a pipelined depth = 0 walk moves on to the next launch ([] = such frames are not held)"""
        arr = np.asarray(list(bounds), dtype=np.int32)
        self.check(self.lib.fs_set_walk_stages(self.h, arr.ctypes.data_as(C.c_void_p) if arr.size else None, int(arr.size)))

    def set_band_edges(self, edges=None):
        """fs_set_band_edges: the num_bands - 1 crossovers (Hz) of FLAG_SPECTRAL_IR's bands; None = the default octave edges"""
        if edges is None:
            self.check(self.lib.fs_set_band_edges(self.h, None, 0))
            return
        arr = np.ascontiguousarray(np.asarray(list(edges), dtype=np.float32))
        self.check(self.lib.fs_set_band_edges(self.h, arr.ctypes.data_as(C.c_void_p) if arr.size else None, int(arr.size)))

    def submit(self):
        self.check(self.lib.fs_submit(self.h))

    def gather_energy_async(self, src: int):
        """enqueue only: (device pointer, bytes) of the gathered [world_size][B][bins] histograms, in tail-stream order"""
        d, b = C.c_void_p(), C.c_size_t()
        self.check(self.lib.fs_gather_energy_async(self.h, int(src), C.byref(d), C.byref(b)))
        return d.value, b.value

    # ---- scene ----
    def set_scene(self, triangles, material_ids, absorption, transmission=None, scattering=None, object_ids=None, fast=False):
        """fast = True: the acceleration structure is built on the device (fs_scene_commit_fast); fast = "progressive": that
        tree now and the host's SAH tree as soon as a background thread has built it (fs_scene_commit_progressive)"""
        tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3)
        mat = np.ascontiguousarray(material_ids, dtype=np.uint16).reshape(-1)
        if mat.shape[0] != tri.shape[0]:
            raise ValueError("material_ids length != number of triangles")
        ab = np.ascontiguousarray(absorption, dtype=np.float32)
        if ab.ndim == 1:
            ab = ab.reshape(-1, 1)
        opt = []
        for a in (transmission, scattering):
            opt.append(None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(ab.shape))
        self.check(self.lib.fs_scene_set_triangles(self.h, tri.ctypes.data, mat.ctypes.data, tri.shape[0]))
        self.check(self.lib.fs_scene_set_materials(self.h, ab.ctypes.data,
                                                   opt[0].ctypes.data if opt[0] is not None else None,
                                                   opt[1].ctypes.data if opt[1] is not None else None,
                                                   ab.shape[0], ab.shape[1]))
        if object_ids is not None:   # actor per triangle (legacy tracer's AddIgnoredActor / pass-through logic)
            obj = np.ascontiguousarray(object_ids, dtype=np.uint32).reshape(-1)
            self.check(self.lib.fs_scene_set_objects(self.h, obj.ctypes.data, obj.shape[0]))
        else:
            self.check(self.lib.fs_scene_set_objects(self.h, None, tri.shape[0]))
        commit = {False: self.lib.fs_scene_commit, True: self.lib.fs_scene_commit_fast,
                  "progressive": self.lib.fs_scene_commit_progressive}[fast]
        self.check(commit(self.h))

    def refine_pending(self) -> bool:
        """fast="progressive": is the background SAH build still outstanding (the swap happens at the next trace after it)"""
        v = C.c_int32(0)
        self.check(self.lib.fs_scene_refine_pending(self.h, C.byref(v)))
        return bool(v.value)

    def refine_wait(self):
        self.check(self.lib.fs_scene_refine_wait(self.h))

    def update_triangles(self, first, triangles):
        """move committed triangles [first, first + n) (row f4: dynamic props); the refit runs before the next trace"""
        t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3)
        self.check(self.lib.fs_scene_update_triangles(self.h, int(first), t.shape[0], t.ctypes.data))

    def refit(self):
        self.check(self.lib.fs_scene_refit(self.h))

    def set_object_transforms(self, ids, matrices):
        """fs_scene_set_object_transforms: every listed actor (ids of set_scene's object_ids) placed at its row-major 3 x 4
        matrix applied to its REST triangles; matrices [n][3][4] or [n][12].  Absolute, not cumulative; enqueues only"""
        o = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1)
        if m.shape[0] != 12 * o.shape[0]:
            raise ValueError("matrices must hold 12 floats per id")
        self.check(self.lib.fs_scene_set_object_transforms(self.h, o.ctypes.data if o.size else None,
                                                           m.ctypes.data if m.size else None, o.shape[0]))

    def set_object_transform(self, object_id, m):
        self.set_object_transforms([int(object_id)], np.asarray(m, dtype=np.float32).reshape(1, 12))

    def set_listener(self, xyz):
        self.check(self.lib.fs_listener_set_position(self.h, _f3(xyz)))

    def create_source(self, xyz=None) -> int:
        s = C.c_int32(-1)
        self.check(self.lib.fs_source_create(self.h, C.byref(s)))
        if xyz is not None:
            self.set_source_position(s.value, xyz)
        return s.value

    def destroy_source(self, src):
        self.check(self.lib.fs_source_destroy(self.h, src))

    def set_source_position(self, src, xyz):
        self.check(self.lib.fs_source_set_position(self.h, src, _f3(xyz)))

    # ---- hot path ----
    def compute_energy_response(self, src, params, want_host=True):
        out = np.empty((self.num_bands, self.num_bins), dtype=np.float32) if want_host else None
        self.check(self.lib.fs_compute_energy_response(self.h, src, C.byref(params),
                                                       out.ctypes.data if want_host else None))
        return out

    def compute_energy_response_async(self, src, params):
        self.check(self.lib.fs_compute_energy_response_async(self.h, src, C.byref(params)))

    def set_source_object(self, src, object_id=_capi.NO_OBJECT):
        """the actor the source belongs to (ids of set_objects): its own walks ignore it (AddIgnoredActor, ARTS.cpp:322-327)"""
        self.check(self.lib.fs_source_set_object(self.h, int(src), int(object_id)))

    def set_listener_object(self, object_id=_capi.NO_OBJECT):
        self.check(self.lib.fs_listener_set_object(self.h, int(object_id)))

    def set_source_orientation(self, src, forward):
        """fs_source_set_orientation: the forward vector the source's directivity table is measured from (default (1, 0, 0))"""
        self.check(self.lib.fs_source_set_orientation(self.h, int(src), _f3(forward)))

    def set_source_directivity(self, src, gains=None):
        """fs_source_set_directivity: gains [bands][samples] (sample k at k pi / (samples - 1) from the forward vector) or
        None (omnidirectional again)"""
        if gains is None:
            self.check(self.lib.fs_source_set_directivity(self.h, int(src), None, 0, 0))
            return
        g = np.ascontiguousarray(gains, dtype=np.float32)
        if g.ndim != 2:
            raise ValueError("gains must be [bands][samples]")
        self.check(self.lib.fs_source_set_directivity(self.h, int(src), g.ctypes.data, g.shape[0], g.shape[1]))

    def set_source_order_window(self, src, min_order=0, max_order=None):
        """fs_source_set_order_window: the source's traced frames deposit only the paths with min_order .. max_order nodes
        made by a hit (both included); max_order None = unbounded, (0, None) = off"""
        hi = _capi.ORDER_UNBOUNDED if max_order is None else int(max_order)
        self.check(self.lib.fs_source_set_order_window(self.h, int(src), int(min_order), hi))

    def source_order_window(self, src):
        """fs_source_get_order_window: (min_order, max_order), max_order None when unbounded"""
        lo, hi = C.c_int32(0), C.c_int32(0)
        self.check(self.lib.fs_source_get_order_window(self.h, int(src), C.byref(lo), C.byref(hi)))
        return int(lo.value), (None if hi.value == _capi.ORDER_UNBOUNDED else int(hi.value))

    def compute_energy_response_batch_async(self, sources, params):
        """several sources in one traced frame (UpdateSource over ActiveSources): same result per source as separate calls"""
        arr = (C.c_int32 * len(sources))(*[int(x) for x in sources])
        self.check(self.lib.fs_compute_energy_response_batch_async(self.h, arr, len(sources), C.byref(params)))

    def reconstruct_impulse_response_batch_async(self, sources, params=None):
        """the tick's reconstructs as one launch with one completion event (same result per source as separate calls)"""
        arr = (C.c_int32 * len(sources))(*[int(x) for x in sources])
        self.check(self.lib.fs_reconstruct_impulse_response_batch_async(self.h, arr, len(sources), C.byref(params) if params else None))

    def update_sources(self, sources, params=None):
        """UpdateSources (ARTS.cpp:100-126): trace + reconstruct every listed source, return when every IR is published"""
        arr = (C.c_int32 * len(sources))(*[int(x) for x in sources])
        self.check(self.lib.fs_update_sources(self.h, arr, len(sources), C.byref(params) if params else None))

    def reconstruct_impulse_response(self, src, params=None):
        self.check(self.lib.fs_reconstruct_impulse_response(self.h, src, C.byref(params) if params else None))

    def reconstruct_impulse_response_async(self, src, params=None):
        self.check(self.lib.fs_reconstruct_impulse_response_async(self.h, src, C.byref(params) if params else None))

    def synchronize(self):
        self.check(self.lib.fs_synchronize(self.h))

    def energy_device_ptr(self, src):
        p, n = C.c_void_p(), C.c_size_t()
        self.check(self.lib.fs_energy_device_ptr(self.h, src, C.byref(p), C.byref(n)))
        return p.value, n.value

    def energy_handoff(self, src):
        """(device pointer, bytes, tail stream handle): the current frame's energy buffer, handed over to the
        tail stream on which the caller's all-reduce and the reconstruct run (include/frequensee.h)"""
        p, n, st = C.c_void_p(), C.c_size_t(), C.c_void_p()
        self.check(self.lib.fs_energy_handoff(self.h, src, C.byref(p), C.byref(n), C.byref(st)))
        return p.value, n.value, st.value

    def impulse_response(self, src, channel=0):
        """copy of the published channel IR (GetImpulseResponse()[channel])"""
        out = np.empty(self.num_samples, dtype=np.float32)
        self.check(self.lib.fs_copy_impulse_response(self.h, src, channel, out.ctypes.data, out.shape[0]))
        return out

    def set_impulse_response(self, src, ir):
        """install an IR of the caller's own (GetImpulseResponse() is a mutable reference, FSAC.h:113)"""
        a = np.ascontiguousarray(ir, dtype=np.float32).reshape(-1)
        self.check(self.lib.fs_set_impulse_response(self.h, src, a.ctypes.data, a.shape[0]))

    def impulse_response_view(self, src, channel=0):
        """zero-copy view of the published front buffer (valid until the second-next publish)"""
        p, n = C.POINTER(C.c_float)(), C.c_int32()
        self.check(self.lib.fs_get_impulse_response(self.h, src, channel, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value,))

    def impulse_response_sequence(self, src):
        """publishes of this source completed so far (the front buffer holds publish number `this` or a newer one)"""
        n = C.c_uint64()
        self.check(self.lib.fs_get_impulse_response_sequence(self.h, src, C.byref(n)))
        return int(n.value)

    ROOM_DTYPE = record_dtype(_capi.RoomParameters)

    def room_parameters(self, src):
        """FS_FLAG_ROOM_PARAMETERS (fs_get_room_parameters): (sequence, structured array [bands] of energy, onset, edt, t20, t30,
        c50, c80, d50, ts) of the front publish; sequence 0 (and an array of NaN) when that publish carries no records"""
        out = np.full(self.num_bands, np.nan, dtype=self.ROOM_DTYPE)
        seq = C.c_uint64()
        self.check(self.lib.fs_get_room_parameters(self.h, int(src), out.ctypes.data_as(C.POINTER(_capi.RoomParameters)),
                                                   self.num_bands, C.byref(seq)))
        return int(seq.value), out

    def band_impulse_response(self, src, band):
        out = np.empty(self.num_samples, dtype=np.float32)
        self.check(self.lib.fs_copy_band_impulse_response(self.h, src, band, out.ctypes.data, out.shape[0]))
        return out

    def update_energy_buffer(self, src, values):
        """UpdateEnergyBuffer (FSAC.h:81-85): install a whole [bands][bins] histogram as the source's current frame"""
        v = np.ascontiguousarray(values, dtype=np.float32)
        self.check(self.lib.fs_update_energy_buffer(self.h, int(src), v.ctypes.data, v.size))

    def energy_buffer(self, src):
        out = np.empty((self.num_bands, self.num_bins), dtype=np.float32)
        self.check(self.lib.fs_get_energy_buffer(self.h, src, out.ctypes.data, out.size))
        return out

    def trace_rays(self, origins, dirs, tmax, any_hit=False):
        """any_hit: False / 0 closest hit, True / 1 any hit, 2 / 3 / 4 closest hit by the cooperative traversal (1 / 2 / 4 rays per wave)"""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        tm = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
        hit = np.zeros(n, dtype=np.int32)
        t = np.zeros(n, dtype=np.float32)
        tri = np.full(n, -1, dtype=np.int32)
        nrm = np.zeros((n, 3), dtype=np.float32)
        self.check(self.lib.fs_trace_rays(self.h, o.ctypes.data, d.ctypes.data, tm.ctypes.data, n, int(any_hit),
                                          hit.ctypes.data, t.ctypes.data, tri.ctypes.data, nrm.ctypes.data))
        return hit.astype(bool), t, tri, nrm

    def update_sound(self, src, params=None):
        """legacy forward tracer UpdateSound (FSAC.cpp:283-306); returns the fs_sound_result fields"""
        r = _capi.SoundResult()
        self.check(self.lib.fs_update_sound(self.h, src, C.byref(params) if params is not None else None, C.byref(r)))
        return r.as_dict()

    def occlusion_attenuation(self, src):
        v = C.c_float()
        self.check(self.lib.fs_get_occlusion_attenuation(self.h, src, C.byref(v)))
        return float(v.value)

    # ---- direct paths: the direct sound of every source of a tick in one launch ----
    DIRECT_DTYPE = record_dtype(_capi.DirectPath)

    @staticmethod
    def direct_sample_offsets(n):
        """fs_direct_sample_offsets: the [n][3] sample offsets (unit sphere, row 0 the centre) direct_paths uses for n samples"""
        out = np.zeros((max(int(n), 0), 3), np.float32)
        rc = _capi.load().fs_direct_sample_offsets(int(n), out.ctypes.data if out.size else None)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_direct_sample_offsets: n must be 1 .. 64")
        return out

    def direct_paths(self, sources, out=None, **params):
        """fs_update_direct_paths: one row per listed source — distance (cm), delay (s), visibility, surfaces the centre ray
        crossed, samples_valid, transmission [8] (bands beyond num_bands: 0) — as a structured array; params = the fields of
        fs_direct_params (samples, source_radius, max_surfaces, step, pullback, dist_divisor, sound_speed)"""
        return self._out_only("direct", sources, params, out)

    def _out_only(self, kind, sources, params, out=None):
        """the body of the out-only queries (PATH_QUERIES rows without a row record): fs_update_<kind>_paths with the given fields
        of its params into `out` or a fresh array [count] of its path record"""
        q = _capi.PATH_QUERY[kind]
        srcs = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        p = _capi.default_path_params(kind, **params)
        if out is None:
            out = np.zeros(srcs.shape[0], dtype=record_dtype(q.path))
        self.check(getattr(self.lib, q.update)(self.h, srcs.ctypes.data if srcs.size else None, int(srcs.shape[0]), C.byref(p),
                                               out.ctypes.data if out.size else None))
        return out

    def _rows_and_paths(self, kind, sources, params):
        """the body of the rows-and-paths queries: fs_update_<kind>_paths with the given fields of its params into fresh
        (rows [count], paths [count][max_paths]) of its two records"""
        q = _capi.PATH_QUERY[kind]
        srcs = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        p = _capi.default_path_params(kind, **params)
        rows = np.zeros(srcs.shape[0], dtype=record_dtype(q.row))
        paths = np.zeros((srcs.shape[0], max(int(p.max_paths), 0)), dtype=record_dtype(q.path))
        self.check(getattr(self.lib, q.update)(self.h, srcs.ctypes.data if srcs.size else None, int(srcs.shape[0]), C.byref(p),
                                               rows.ctypes.data if rows.size else None, paths.ctypes.data if paths.size else None))
        return rows, paths

    # ---- reflection paths: the first-order specular reflections of every source of a tick ----
    REFLECTION_ROW_DTYPE = record_dtype(_capi.ReflectionRow)
    REFLECTION_DTYPE = record_dtype(_capi.ReflectionPath)

    def reflection_paths(self, sources, **params):
        """fs_update_reflection_paths: (rows [count], paths [count][max_paths]) as structured arrays — per listed source the counts
        (candidates, found, returned, flags) and its `returned` shortest reflections (length cm, delay s, point, direction from the
        listener, triangle, material, reflectance [8]; entries beyond `returned` are zero); params = the fields of
        fs_reflection_params (max_paths, max_candidates, margin, step, offset, pullback, dist_divisor, sound_speed)"""
        return self._rows_and_paths("reflection", sources, params)

    # ---- diffraction paths: the first-order edge diffraction of every source of a tick ----
    DIFFRACTION_ROW_DTYPE = record_dtype(_capi.DiffractionRow)
    DIFFRACTION_DTYPE = record_dtype(_capi.DiffractionPath)

    def diffraction_paths(self, sources, **params):
        """fs_update_diffraction_paths: (rows [count], paths [count][max_paths]) as structured arrays — per listed source the counts
        (candidates, confirmed, found, returned, flags) and its `returned` shortest paths round one edge (length cm, delay s, detour
        cm, cos_bend, apex, direction from the listener, triangle, edge, material, gain [8]; entries beyond `returned` are zero);
        params = the fields of fs_diffraction_params (max_paths, max_candidates, margin, max_detour, offset, merge, step, pullback,
        dist_divisor, sound_speed)"""
        return self._rows_and_paths("diffraction", sources, params)

    # ---- second-order reflection paths: the specular reflections off two triangles of every source of a tick ----
    REFLECTION2_ROW_DTYPE = record_dtype(_capi.Reflection2Row)
    REFLECTION2_DTYPE = record_dtype(_capi.Reflection2Path)

    def reflection2_paths(self, sources, **params):
        """fs_update_reflection2_paths: (rows [count], paths [count][max_paths]) as structured arrays — per listed source the counts
        (near, candidates, found, returned, flags) and its `returned` shortest paths listener -> PA on triangle a -> PB on triangle b
        -> source (length cm, delay s, point [PA, PB], direction from the listener, triangle [a, b], material [2], reflectance [8];
        entries beyond `returned` are zero); params = the fields of fs_reflection2_params (max_paths, max_near, max_candidates,
        max_length, margin, step, offset, pullback, dist_divisor, sound_speed)"""
        return self._rows_and_paths("reflection2", sources, params)

    # ---- second-order diffraction paths: the diffraction round thick obstacles of every source of a tick ----
    DIFFRACTION2_ROW_DTYPE = record_dtype(_capi.Diffraction2Row)
    DIFFRACTION2_DTYPE = record_dtype(_capi.Diffraction2Path)

    def diffraction2_paths(self, sources, **params):
        """fs_update_diffraction2_paths: (rows [count], paths [count][max_paths]) as structured arrays — per listed source the counts
        (near, candidates, confirmed, found, returned, flags) and its `returned` shortest paths listener -> E0 -> E1 -> source round
        two parallel edges (length cm, delay s, detour cm, gap cm, cos_bend [2], apex [E0, E1], direction from the listener,
        triangle [2], edge [2], material [2], gain [8]; index 0 is the listener's end; entries beyond `returned` are zero);
        params = the fields of fs_diffraction2_params (max_paths, max_near, max_candidates, margin, max_detour, min_parallel, offset,
        merge, step, pullback, dist_divisor, sound_speed)"""
        return self._rows_and_paths("diffraction2", sources, params)

    # ---- mixed paths: one specular reflection and one edge diffraction of every source of a tick ----
    MIXED_ROW_DTYPE = record_dtype(_capi.MixedRow)
    MIXED_DTYPE = record_dtype(_capi.MixedPath)

    def mixed_paths(self, sources, **params):
        """fs_update_mixed_paths: (rows [count], paths [count][max_paths]) as structured arrays — per listed source the counts
        (near, candidates, confirmed, found, returned, flags) and its `returned` shortest paths off one reflector and round one
        edge (length cm, delay s, detour cm, bend_detour cm, cos_bend, apex E, point R, direction from the listener, end — 0: the
        reflector is next to the listener, 1: next to the source —, triangle [reflector, the edge's], edge, material [2], gain [8];
        entries beyond `returned` are zero); params = the fields of fs_mixed_params (max_paths, max_near, max_candidates,
        max_length, max_detour, margin, offset, merge, step, pullback, dist_divisor, sound_speed)"""
        return self._rows_and_paths("mixed", sources, params)

    # ---- pathing: round several corners by a probe graph ----
    PATHING_DTYPE = record_dtype(_capi.PathingPath)

    def pathing_set_probes(self, xyz=None):
        """fs_pathing_set_probes: the probe set, [count][3] points in free air (cm); None or an empty array clears it.  Drops any bake"""
        a = np.zeros((0, 3), np.float32) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self.check(self.lib.fs_pathing_set_probes(self.h, a.ctypes.data if a.size else None, int(a.shape[0])))

    def pathing_bake(self, **params):
        """fs_pathing_bake: which pairs of probes see each other; params = the fields of fs_pathing_bake_params (max_edge, step).
        Returns the number of undirected edges"""
        p = _capi.default_pathing_bake_params(**params)
        self.check(self.lib.fs_pathing_bake(self.h, C.byref(p)))
        return self.pathing_info()["edges"]

    def pathing_info(self):
        """fs_pathing_info: dict(probes, edges, baked, scene_changed)"""
        v = [C.c_int32() for _ in range(4)]
        self.check(self.lib.fs_pathing_info(self.h, *[C.byref(x) for x in v]))
        return dict(probes=v[0].value, edges=v[1].value, baked=bool(v[2].value), scene_changed=bool(v[3].value))

    def pathing_graph(self):
        """fs_pathing_copy_graph: the baked graph as uint32 [N][ceil(N / 32)], bit (j & 31) of word (j >> 5) of row i = {i, j} is an edge"""
        n = self.pathing_info()["probes"]
        out = np.zeros((n, (n + 31) // 32), np.uint32)
        self.check(self.lib.fs_pathing_copy_graph(self.h, out.ctypes.data if out.size else None, int(out.size)))
        return out

    def pathing_paths(self, sources, **params):
        """fs_update_pathing_paths: one row per listed source as a structured array — length (cm), delay (s), detour, distance,
        direction (from the listener towards the first probe), departure (from the source towards the last), hops, flags
        (PATHING_FOUND | PATHING_DIRECT | PATHING_STALE), first_probe, last_probe, probes [16] from the listener's end, gain [8];
        params = the fields of fs_pathing_params (validate, max_attach, max_length, step, pullback, dist_divisor, sound_speed)"""
        return self._out_only("pathing", sources, params)

    # ---- the audio callbacks: what the three *_process_batch mirrors share ----
    def _callback_open(self, sources, blocks, frames, want_out, want_mix):
        """the opening of a callback: (handles, count, blocks [count][frame_size * 2], out or None, mix or None); frames = the
        frame size each initialised source was given"""
        srcs = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        count = int(srcs.shape[0])
        a = np.ascontiguousarray(blocks, dtype=np.float32).reshape(count, -1) if count else np.zeros((0, 0), np.float32)
        if count and int(srcs[0]) in frames and a.shape[1] != 2 * frames[int(srcs[0])]:
            raise ValueError("every audio block must hold frame_size * 2 interleaved samples")
        return srcs, count, a, np.empty_like(a) if want_out else None, np.empty(a.shape[1], np.float32) if want_mix else None

    @staticmethod
    def _callback_close(*results):
        """the close: what was asked for (not None) — alone, or as a tuple when there is more than one"""
        got = tuple(x for x in results if x is not None)
        return got if len(got) > 1 else got[0]

    @staticmethod
    def _voice_table(voices, count, stride, dtype, write):
        """a voice-bank callback's (table [count][stride] of dtype, counts [count], stride) from one list per source, each an
        array of dtype or tuples; write(entry, tuple) puts what the renderer's tuple holds beyond (key, delay, band_gain) into the
        entry and returns those three"""
        if len(voices) != count:
            raise ValueError("voices must have one list per source")
        if stride is None:
            stride = max([len(v) for v in voices] + [1])
        stride = int(stride)
        if any(len(v) > stride for v in voices):
            raise ValueError("a voice list is longer than stride")
        table = np.zeros((count, max(stride, 1)), dtype=dtype)
        counts = np.zeros(count, np.int32)
        for i, lst in enumerate(voices):
            counts[i] = len(lst)
            if isinstance(lst, np.ndarray) and lst.dtype == dtype:
                table[i, :len(lst)] = lst
                continue
            for e, entry in enumerate(lst):
                key, delay, gains = write(table[i, e], entry)
                g = np.asarray(gains, np.float32).reshape(-1)
                table[i, e]["key"] = key
                table[i, e]["delay"] = delay
                table[i, e]["band_gain"][:g.shape[0]] = g
        return table, counts, stride

    # ---- direct sound on the audio thread: fractional delay + band FIR for all sources of a callback ----
    RENDER_TARGET_DTYPE = record_dtype(_capi.DirectRenderTarget)

    @staticmethod
    def direct_band_kernels(sample_rate, bands, taps, edges=None):
        """fs_direct_band_kernels: the [bands][taps] band kernels (edges: the bands - 1 inner edges in Hz, None = the default
        octave edges); with the context's sample rate, band count and edges it is the table direct_render_init uploads"""
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float32).reshape(-1)
        if e is not None and e.shape[0] != max(int(bands) - 1, 0):
            raise ValueError("edges must hold bands - 1 values")
        out = np.zeros((max(int(bands), 0), max(int(taps), 0)), np.float32)
        rc = _capi.load().fs_direct_band_kernels(int(sample_rate), e.ctypes.data if e is not None and e.size else None, int(bands),
                                                 int(taps), out.ctypes.data if out.size else None)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_direct_band_kernels: bands 1 .. 8, taps odd 1 .. 2047, edges ascending inside (0, sample_rate / 2)")
        return out

    def direct_render_init(self, src, frame_size=1024, taps=255, max_delay_seconds=1.0):
        self.check(self.lib.fs_direct_render_init(self.h, src, int(frame_size), int(taps), float(max_delay_seconds)))
        self._dr_frame = getattr(self, "_dr_frame", {})
        self._dr_frame[src] = int(frame_size)

    def direct_render_release(self, src):
        self.check(self.lib.fs_direct_render_release(self.h, src))

    def direct_render_process_batch(self, sources, blocks, targets, want_out=True, want_mix=False):
        """the direct sound of several sources as one set of launches (include/frequensee.h fs_direct_render_process_batch):
        blocks [count][frame_size * 2], targets a RENDER_TARGET_DTYPE array or (delay, band_gain) pairs -> out
        [count][frame_size * 2] (want_out), mix [frame_size * 2] (want_mix), or the pair (out, mix)"""
        srcs, count, a, out, mix = self._callback_open(sources, blocks, getattr(self, "_dr_frame", {}), want_out, want_mix)
        if isinstance(targets, np.ndarray) and targets.dtype == self.RENDER_TARGET_DTYPE:
            t = np.ascontiguousarray(targets).reshape(-1)
        else:
            t = np.zeros(len(targets), dtype=self.RENDER_TARGET_DTYPE)
            for i, (delay, gains) in enumerate(targets):
                g = np.asarray(gains, np.float32).reshape(-1)
                t[i]["delay"] = delay
                t[i]["band_gain"][:g.shape[0]] = g
        if t.shape[0] != count:
            raise ValueError("targets must have one entry per source")
        self.check(self.lib.fs_direct_render_process_batch(self.h, srcs.ctypes.data, count, a.ctypes.data, t.ctypes.data,
                                                           out.ctypes.data if want_out else None, mix.ctypes.data if want_mix else None))
        return self._callback_close(out, mix)

    # ---- early reflections on the audio thread: a bank of delayed, filtered, panned voices per source ----
    REFLECTION_VOICE_DTYPE = record_dtype(_capi.ReflectionVoice)
    REFLECTION_RENDER_ROW_DTYPE = record_dtype(_capi.ReflectionRenderRow)

    def reflection_render_init(self, src, frame_size=1024, taps=255, voices=32, max_delay_seconds=1.0):
        self.check(self.lib.fs_reflection_render_init(self.h, src, int(frame_size), int(taps), int(voices), float(max_delay_seconds)))
        self._rr_frame = getattr(self, "_rr_frame", {})
        self._rr_frame[src] = int(frame_size)

    def reflection_render_release(self, src):
        self.check(self.lib.fs_reflection_render_release(self.h, src))

    def reflection_render_process_batch(self, sources, blocks, voices, stride=None, want_out=True, want_mix=False):
        """the early reflections of several sources as one set of launches (include/frequensee.h
        fs_reflection_render_process_batch): blocks [count][frame_size * 2]; voices one list per source, each a
        REFLECTION_VOICE_DTYPE array or (key, delay, band_gain, channel_gain) tuples; stride = the row length handed to the library
        (default: the longest list, at least 1) -> (out [count][frame_size * 2] (want_out), mix [frame_size * 2] (want_mix), rows
        [count] REFLECTION_RENDER_ROW_DTYPE); what was not asked for is left out of the tuple"""
        srcs, count, a, out, mix = self._callback_open(sources, blocks, getattr(self, "_rr_frame", {}), want_out, want_mix)

        def write(entry, voice):
            key, delay, gains, chan = voice
            entry["channel_gain"] = chan
            return key, delay, gains

        table, counts, stride = self._voice_table(voices, count, stride, self.REFLECTION_VOICE_DTYPE, write)
        rows = np.zeros(count, dtype=self.REFLECTION_RENDER_ROW_DTYPE)
        self.check(self.lib.fs_reflection_render_process_batch(self.h, srcs.ctypes.data, count, a.ctypes.data, table.ctypes.data,
                                                               counts.ctypes.data, stride, out.ctypes.data if want_out else None,
                                                               mix.ctypes.data if want_mix else None, rows.ctypes.data))
        return self._callback_close(out, mix, rows)

    # ---- binaural voices on the audio thread: the voice bank with a direction per voice and an HRIR set per context ----
    BINAURAL_VOICE_DTYPE = record_dtype(_capi.BinauralVoice)
    BINAURAL_RENDER_ROW_DTYPE = record_dtype(_capi.BinauralRenderRow)

    @staticmethod
    def hrtf_spherical_head(sample_rate, directions, taps, radius_cm=_capi.HRTF_DEFAULT_RADIUS_CM,
                            sound_speed_cm_s=_capi.HRTF_DEFAULT_SOUND_SPEED_CM_S):
        """fs_hrtf_spherical_head: (dirs [directions][3], hrir [directions][2][taps]) of the header's spherical-head model — a
        model: interaural delay and level difference, no pinna"""
        n, H = max(int(directions), 0), max(int(taps), 0)
        dirs, hrir = np.zeros((n, 3), np.float32), np.zeros((n, 2, H), np.float32)
        rc = _capi.load().fs_hrtf_spherical_head(int(sample_rate), float(radius_cm), float(sound_speed_cm_s), int(directions), int(taps),
                                                 dirs.ctypes.data if dirs.size else None, hrir.ctypes.data if hrir.size else None)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_hrtf_spherical_head: directions 1 .. 4096, taps 1 .. 512 and at least ceil((a / c)(1 + pi / 2) fs) + 2, "
                                      "positive finite radius and sound speed")
        return dirs, hrir

    def hrtf_set(self, dirs, hrir, sample_rate=None):
        """fs_hrtf_set: dirs [n][3] unit vectors in the head frame (x forward, y right, z up), hrir [n][2][H] (ear 0 left);
        dirs = None clears the set.  Not concurrent with a callback; every held binaural voice starts anew afterwards"""
        if dirs is None:
            self.check(self.lib.fs_hrtf_set(self.h, None))
            return
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        h = np.ascontiguousarray(hrir, dtype=np.float32)
        if d.ndim != 2 or d.shape[1] != 3 or h.ndim != 3 or h.shape[:2] != (d.shape[0], 2):
            raise ValueError("dirs must be [n][3] and hrir [n][2][H]")
        desc = _capi.HrtfDesc()
        desc.struct_size = C.sizeof(_capi.HrtfDesc)
        desc.directions, desc.taps = d.shape[0], h.shape[2]
        desc.sample_rate = int(self.cfg.sample_rate if sample_rate is None else sample_rate)
        desc.dirs, desc.hrir = d.ctypes.data, h.ctypes.data
        self.check(self.lib.fs_hrtf_set(self.h, C.byref(desc)))

    def hrtf_info(self):
        """(directions, taps) of the set in force, (0, 0) without one"""
        n, H = C.c_int32(-1), C.c_int32(-1)
        self.check(self.lib.fs_hrtf_info(self.h, C.byref(n), C.byref(H)))
        return n.value, H.value

    @staticmethod
    def hrtf_triangulate(dirs):
        """fs_hrtf_triangulate: tri [2n - 4][3] int32, the convex hull of dirs [n][3] as a mesh fs_hrtf_mesh_rows accepts (host only)"""
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError("dirs must be [n][3]")
        n = d.shape[0]
        tri = np.zeros((max(2 * n - 4, 0), 3), np.int32)
        m = C.c_int32(0)
        rc = _capi.load().fs_hrtf_triangulate(d.ctypes.data if d.size else None, n, tri.ctypes.data if tri.size else None, tri.shape[0], C.byref(m))
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_hrtf_triangulate: 4 .. 4096 finite, distinct directions that surround the origin")
        return tri[:m.value]

    @staticmethod
    def hrtf_mesh_rows(dirs, tri):
        """fs_hrtf_mesh_rows: rows [m][3][3] float32 of the mesh tri [m][3] on dirs [n][3] — r_i . d are the coefficients of d in
        the triangle's corners; raises where the mesh is refused (host only)"""
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        t = np.ascontiguousarray(tri, dtype=np.int32)
        if d.ndim != 2 or d.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("dirs must be [n][3] and tri [m][3]")
        rows = np.zeros((t.shape[0], 3, 3), np.float32)
        rc = _capi.load().fs_hrtf_mesh_rows(d.ctypes.data if d.size else None, d.shape[0], t.ctypes.data if t.size else None, t.shape[0],
                                            rows.ctypes.data if rows.size else None)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_hrtf_mesh_rows: not a closed, outward-facing triangulation of 2n - 4 triangles on all n directions")
        return rows

    @staticmethod
    def hrtf_mesh_locate(rows, direction):
        """fs_hrtf_mesh_locate: (t, b [3] float32) — the triangle a direction falls in and its weights, the bits the device computes"""
        r = np.ascontiguousarray(rows, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32).reshape(-1)
        if r.ndim != 3 or r.shape[1:] != (3, 3) or d.shape[0] != 3:
            raise ValueError("rows must be [m][3][3] and direction hold three components")
        t, b = C.c_int32(-1), np.zeros(3, np.float32)
        rc = _capi.load().fs_hrtf_mesh_locate(r.ctypes.data if r.size else None, r.shape[0], d.ctypes.data, C.byref(t), b.ctypes.data)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_hrtf_mesh_locate: at least one triangle")
        return t.value, b

    def hrtf_set_mesh(self, tri):
        """fs_hrtf_set_mesh: tri [m][3] on the set in force, validated as fs_hrtf_mesh_rows does; None clears the mesh.  Not
        concurrent with a callback; every held binaural voice starts anew afterwards"""
        if tri is None:
            self.check(self.lib.fs_hrtf_set_mesh(self.h, None, 0))
            return
        t = np.ascontiguousarray(tri, dtype=np.int32)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("tri must be [m][3]")
        self.check(self.lib.fs_hrtf_set_mesh(self.h, t.ctypes.data if t.size else None, t.shape[0]))

    def hrtf_mesh_info(self):
        """the triangles of the mesh in force, 0 without one"""
        m = C.c_int32(-1)
        self.check(self.lib.fs_hrtf_mesh_info(self.h, C.byref(m)))
        return m.value

    def hrtf_set_onsets(self, onsets):
        """fs_hrtf_set_onsets: onsets [n][2] in samples on the set in force, whose HRIRs are then read as aligned — a voice's HRIR
        is delayed by its own onset, with a mesh the blend of the corners'; None clears them.  Not concurrent with a callback;
        every held binaural voice starts anew afterwards"""
        if onsets is None:
            self.check(self.lib.fs_hrtf_set_onsets(self.h, None))
            return
        o = np.ascontiguousarray(onsets, dtype=np.float32)
        if o.ndim != 2 or o.shape != (self.hrtf_info()[0], 2):
            raise ValueError("onsets must be [n][2] for the n directions of the set in force")
        self.check(self.lib.fs_hrtf_set_onsets(self.h, o.ctypes.data if o.size else None))

    def hrtf_onsets_info(self):
        """(installed, extra_taps): whether onsets are in force, and O = (int)omax + 1 — a delayed HRIR has H + O taps"""
        on, extra = C.c_int32(-1), C.c_int32(-1)
        self.check(self.lib.fs_hrtf_onsets_info(self.h, C.byref(on), C.byref(extra)))
        return bool(on.value), extra.value

    @staticmethod
    def hrtf_delay(h, tau, taps=None):
        """fs_hrtf_delay: h [H] delayed by tau samples with the header's linear fractional delay, as `taps` taps (by default
        H + (int)tau + 1, the fewest that hold it) — the bits the device computes (host only)"""
        x = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
        tau = float(np.float32(tau))   # (what the library is handed)
        if taps is None:
            taps = x.shape[0] + int(tau) + 1 if np.isfinite(tau) and 0.0 <= tau < 2.0 ** 30 else 0
        out = np.zeros(max(int(taps), 0), np.float32)
        rc = _capi.load().fs_hrtf_delay(x.ctypes.data if x.size else None, x.shape[0], tau, out.ctypes.data if out.size else None, int(taps))
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_hrtf_delay: at least one tap, a finite delay >= 0 and room for H + (int)tau + 1 taps")
        return out

    @staticmethod
    def hrtf_split_onsets(hrir, threshold=0.1, lead=0):
        """fs_hrtf_split_onsets: (aligned [n][2][H], onsets [n][2]) of a set that comes without delays — per direction and ear the
        onset is the first tap at `threshold` of the peak, less `lead`, and the HRIR is moved up by it (host only)"""
        h = np.ascontiguousarray(hrir, dtype=np.float32)
        if h.ndim != 3 or h.shape[1] != 2:
            raise ValueError("hrir must be [n][2][H]")
        aligned, onsets = np.zeros_like(h), np.zeros(h.shape[:2], np.float32)
        rc = _capi.load().fs_hrtf_split_onsets(h.ctypes.data if h.size else None, h.shape[0], h.shape[2], float(threshold), int(lead),
                                               aligned.ctypes.data if aligned.size else None, onsets.ctypes.data if onsets.size else None)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_hrtf_split_onsets: at least one direction and tap, threshold in (0, 1], lead >= 0")
        return aligned, onsets

    @staticmethod
    def hrtf_spherical_head_split(sample_rate, directions, taps, radius_cm=_capi.HRTF_DEFAULT_RADIUS_CM,
                                  sound_speed_cm_s=_capi.HRTF_DEFAULT_SOUND_SPEED_CM_S):
        """fs_hrtf_spherical_head_split: (dirs [directions][3], hrir [directions][2][taps], onsets [directions][2]) — the
        spherical-head model with the shadow filter and the onset handed out apart, for fs_hrtf_set and fs_hrtf_set_onsets"""
        n, H = max(int(directions), 0), max(int(taps), 0)
        dirs, hrir, onsets = np.zeros((n, 3), np.float32), np.zeros((n, 2, H), np.float32), np.zeros((n, 2), np.float32)
        rc = _capi.load().fs_hrtf_spherical_head_split(int(sample_rate), float(radius_cm), float(sound_speed_cm_s), int(directions), int(taps),
                                                       dirs.ctypes.data if dirs.size else None, hrir.ctypes.data if hrir.size else None,
                                                       onsets.ctypes.data if onsets.size else None)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_hrtf_spherical_head_split: directions 1 .. 4096, taps 2 .. 512, positive finite radius and sound speed")
        return dirs, hrir, onsets

    def binaural_render_init(self, src, frame_size=1024, taps=255, voices=32, max_delay_seconds=1.0):
        self.check(self.lib.fs_binaural_render_init(self.h, src, int(frame_size), int(taps), int(voices), float(max_delay_seconds)))
        self._br_frame = getattr(self, "_br_frame", {})
        self._br_frame[src] = int(frame_size)

    def binaural_render_release(self, src):
        self.check(self.lib.fs_binaural_render_release(self.h, src))

    def binaural_render_process_batch(self, sources, blocks, voices, stride=None, want_out=True, want_mix=False):
        """the binaural voices of several sources as one set of launches (include/frequensee.h
        fs_binaural_render_process_batch): blocks [count][frame_size * 2]; voices one list per source, each a
        BINAURAL_VOICE_DTYPE array or (key, delay, band_gain, gain, direction) tuples; stride = the row length handed to the
        library (default: the longest list, at least 1) -> (out [count][frame_size * 2] (want_out), mix [frame_size * 2]
        (want_mix), rows [count] BINAURAL_RENDER_ROW_DTYPE); what was not asked for is left out of the tuple"""
        srcs, count, a, out, mix = self._callback_open(sources, blocks, getattr(self, "_br_frame", {}), want_out, want_mix)

        def write(entry, voice):
            key, delay, gains, gain, direction = voice
            entry["gain"] = gain
            entry["direction"] = direction
            return key, delay, gains

        table, counts, stride = self._voice_table(voices, count, stride, self.BINAURAL_VOICE_DTYPE, write)
        rows = np.zeros(count, dtype=self.BINAURAL_RENDER_ROW_DTYPE)
        self.check(self.lib.fs_binaural_render_process_batch(self.h, srcs.ctypes.data, count, a.ctypes.data, table.ctypes.data,
                                                             counts.ctypes.data, stride, out.ctypes.data if want_out else None,
                                                             mix.ctypes.data if want_mix else None, rows.ctypes.data))
        return self._callback_close(out, mix, rows)

    # ---- ambisonic voices on the audio thread: the voice bank with a direction per voice, rendered into a soundfield ----
    AMBISONIC_VOICE_DTYPE = BINAURAL_VOICE_DTYPE   # fs_ambisonic_voice is fs_binaural_voice
    AMBISONIC_RENDER_ROW_DTYPE = record_dtype(_capi.AmbisonicRenderRow)

    @staticmethod
    def ambisonic_encode(order, direction):
        """fs_ambisonic_encode: the (order + 1)^2 channel gains of a direction in the head frame (x forward, y right, z up), ACN
        order and SN3D normalisation, fp32 — the bits the renderer's plan pass computes on the device"""
        d = np.ascontiguousarray(direction, dtype=np.float32).reshape(-1)
        if d.shape[0] != 3:
            raise ValueError("direction must hold three components")
        out = np.zeros((min(max(int(order), 0), _capi.MAX_AMBISONIC_ORDER) + 1) ** 2, np.float32)
        rc = _capi.load().fs_ambisonic_encode(int(order), d.ctypes.data, out.ctypes.data)
        if rc != _capi.OK:
            raise FrequenSeeError(rc, "fs_ambisonic_encode: order 0 .. 3, a finite direction whose squared length lies in 1e-30 .. 1e30")
        return out

    def ambisonic_render_init(self, src, frame_size=1024, taps=255, voices=32, max_delay_seconds=1.0, order=1):
        self.check(self.lib.fs_ambisonic_render_init(self.h, src, int(frame_size), int(taps), int(voices), float(max_delay_seconds), int(order)))
        self._ar_frame = getattr(self, "_ar_frame", {})
        self._ar_order = getattr(self, "_ar_order", {})
        self._ar_frame[src] = int(frame_size)
        self._ar_order[src] = int(order)

    def ambisonic_render_release(self, src):
        self.check(self.lib.fs_ambisonic_render_release(self.h, src))

    def ambisonic_render_process_batch(self, sources, blocks, voices, stride=None, want_out=True, want_mix=False):
        """the ambisonic voices of several sources as one set of launches (include/frequensee.h
        fs_ambisonic_render_process_batch): blocks [count][frame_size * 2]; voices one list per source, each an
        AMBISONIC_VOICE_DTYPE array or (key, delay, band_gain, gain, direction) tuples; stride = the row length handed to the
        library (default: the longest list, at least 1) -> (out [count][frame_size][C] (want_out), mix [frame_size][C]
        (want_mix), rows [count] AMBISONIC_RENDER_ROW_DTYPE), C = (order + 1)^2 of the order the first source was initialised
        with; what was not asked for is left out of the tuple"""
        srcs, count, a, _, _ = self._callback_open(sources, blocks, getattr(self, "_ar_frame", {}), False, False)
        order = max([getattr(self, "_ar_order", {}).get(int(s), 0) for s in srcs] + [0])   # (sources of unlike orders are refused)
        frame, channels = a.shape[1] // 2, (order + 1) ** 2
        out = np.empty((count, frame, channels), np.float32) if want_out else None
        mix = np.empty((frame, channels), np.float32) if want_mix else None

        def write(entry, voice):
            key, delay, gains, gain, direction = voice
            entry["gain"] = gain
            entry["direction"] = direction
            return key, delay, gains

        table, counts, stride = self._voice_table(voices, count, stride, self.AMBISONIC_VOICE_DTYPE, write)
        rows = np.zeros(count, dtype=self.AMBISONIC_RENDER_ROW_DTYPE)
        self.check(self.lib.fs_ambisonic_render_process_batch(self.h, srcs.ctypes.data, count, a.ctypes.data, table.ctypes.data,
                                                              counts.ctypes.data, stride, out.ctypes.data if want_out else None,
                                                              mix.ctypes.data if want_mix else None, rows.ctypes.data))
        return self._callback_close(out, mix, rows)

    # ---- row f2: reverb plugin convolution ----
    def reverb_init(self, src, frame_size=1024):
        self.check(self.lib.fs_reverb_init(self.h, src, frame_size))
        self._rev_frame = getattr(self, "_rev_frame", {})
        self._rev_frame[src] = frame_size

    def reverb_process(self, src, audio_interleaved, apply_reverb=True, literal_tail=False):
        """ProcessSourceAudio (RVB.cpp:118-170): interleaved stereo block in -> convolved block out"""
        frame = self._rev_frame[src]
        a = np.ascontiguousarray(audio_interleaved, dtype=np.float32).reshape(-1)
        if a.shape[0] != 2 * frame:
            raise ValueError("audio block must hold frame_size * 2 interleaved samples")
        out = np.empty_like(a)
        self.check(self.lib.fs_reverb_process(self.h, src, a.ctypes.data, out.ctypes.data, int(apply_reverb),
                                              _capi.REVERB_LITERAL_TAIL if literal_tail else 0))
        return out

    def reverb_process_batch(self, sources, blocks, apply=None, literal_tail=False, want_out=True, want_mix=False):
        """the callbacks of several sources as one set of launches (include/frequensee.h fs_reverb_process_batch):
        blocks [count][frame_size * 2] -> out [count][frame_size * 2] (want_out), mix [frame_size * 2] (want_mix: the fp32 sum of
        the outputs in list order), or the pair (out, mix) when both are asked for"""
        srcs, count, a, out, mix = self._callback_open(sources, blocks, getattr(self, "_rev_frame", {}), want_out, want_mix)
        on = None
        if apply is not None:
            on = np.ascontiguousarray([1 if x else 0 for x in apply], dtype=np.int32)
            if on.shape[0] != count:
                raise ValueError("apply must have one entry per source")
        self.check(self.lib.fs_reverb_process_batch(self.h, srcs.ctypes.data, count, a.ctypes.data,
                                                    out.ctypes.data if want_out else None, on.ctypes.data if on is not None else None,
                                                    _capi.REVERB_LITERAL_TAIL if literal_tail else 0,
                                                    mix.ctypes.data if want_mix else None))
        return self._callback_close(out, mix)

    def reverb_release(self, src):
        self.check(self.lib.fs_reverb_release(self.h, src))

    def reverb_set_crossfade(self, src, samples):
        """crossfade the callback between successive IRs over `samples` output samples (0: off, the reference's abrupt
        switch; include/frequensee.h fs_reverb_set_crossfade)"""
        self.check(self.lib.fs_reverb_set_crossfade(self.h, src, int(samples)))

    def reverb_set_engine(self, src, engine):
        """the engine the source's next reverb_init gives it: _capi.REVERB_ENGINE_DIRECT (the default, tap by tap) or
        _capi.REVERB_ENGINE_PARTITIONED (partitioned FFT convolution: no limit from the history ring, a cost that hardly
        grows with the IR; include/frequensee.h fs_reverb_set_engine)"""
        self.check(self.lib.fs_reverb_set_engine(self.h, src, int(engine)))

    def reverb_ears_set(self, radius_cm=None, sound_speed_cm_s=None, clear=False):
        """fs_reverb_ears_set: build and install the two-ear reverb's carriers (diffuse-field coherence of two points 2 radius_cm
        apart; None = the spherical head's defaults), or clear the set (include/frequensee.h "Two-ear late reverb")"""
        if clear:
            self.check(self.lib.fs_reverb_ears_set(self.h, None))
            return
        kw = {}
        if radius_cm is not None:
            kw["radius_cm"] = float(radius_cm)
        if sound_speed_cm_s is not None:
            kw["sound_speed_cm_s"] = float(sound_speed_cm_s)
        d = _capi.default_reverb_ears(**kw)
        self.check(self.lib.fs_reverb_ears_set(self.h, C.byref(d)))

    def reverb_ears_info(self):
        """fs_reverb_ears_info -> (radius_cm, sound_speed_cm_s, installed)"""
        r, c, on = C.c_float(0.0), C.c_float(0.0), C.c_int32(0)
        self.check(self.lib.fs_reverb_ears_info(self.h, C.addressof(r), C.addressof(c), C.addressof(on)))
        return float(r.value), float(c.value), bool(on.value)

    def reverb_set_ears(self, src, on):
        """ears for the source's next reverb_init (needs the partitioned engine and an installed set there)"""
        self.check(self.lib.fs_reverb_set_ears(self.h, src, 1 if on else 0))

    def reverb_ear_impulse_responses(self, src):
        """fs_reverb_copy_ear_impulse_responses -> (left, right): h_L and h_R of the source's newest device-resident IR"""
        left = np.empty(self.num_samples, dtype=np.float32)
        right = np.empty(self.num_samples, dtype=np.float32)
        self.check(self.lib.fs_reverb_copy_ear_impulse_responses(self.h, src, left.ctypes.data, right.ctypes.data, left.shape[0]))
        return left, right

    def reverb_soundfield_set(self, order=1, clear=False):
        """fs_reverb_soundfield_set: build and install the soundfield reverb's carriers for an ACN/SN3D bus of (order + 1)^2
        channels, or clear the set (include/frequensee.h "soundfield late reverb")"""
        self.check(self.lib.fs_reverb_soundfield_set(self.h, -1 if clear else int(order)))

    def reverb_soundfield_info(self):
        """fs_reverb_soundfield_info -> (order, installed); order is -1 with no set installed"""
        order, on = C.c_int32(0), C.c_int32(0)
        self.check(self.lib.fs_reverb_soundfield_info(self.h, C.addressof(order), C.addressof(on)))
        return int(order.value), bool(on.value)

    def reverb_set_soundfield(self, src, on):
        """the soundfield for the source's next reverb_init (needs the partitioned engine, an installed set and no ears there)"""
        self.check(self.lib.fs_reverb_set_soundfield(self.h, src, 1 if on else 0))

    def reverb_soundfield_impulse_responses(self, src):
        """fs_reverb_copy_soundfield_impulse_responses -> [C][num_samples]: h_c of the source's newest device-resident IR"""
        order, on = self.reverb_soundfield_info()
        out = np.empty(((order + 1) ** 2 if on else 1, self.num_samples), dtype=np.float32)
        self.check(self.lib.fs_reverb_copy_soundfield_impulse_responses(self.h, src, out.ctypes.data, out.shape[1]))
        return out

    def reverb_soundfield_process_batch(self, sources, blocks, want_out=True, want_mix=False, flags=0):
        """the soundfield callbacks of several sources as one set of launches (include/frequensee.h
        fs_reverb_soundfield_process_batch): blocks [count][frame_size * 2] -> out [count][frame_size][C] (want_out), mix
        [frame_size][C] (want_mix: the fp32 sum of the outputs in list order), or the pair when both are asked for; C = (order +
        1)^2 of the set installed"""
        srcs, count, a, _, _ = self._callback_open(sources, blocks, getattr(self, "_rev_frame", {}), False, False)
        order, _ = self.reverb_soundfield_info()
        frame, channels = a.shape[1] // 2, (max(order, 0) + 1) ** 2
        out = np.empty((count, frame, channels), np.float32) if want_out else None
        mix = np.empty((frame, channels), np.float32) if want_mix else None
        self.check(self.lib.fs_reverb_soundfield_process_batch(self.h, srcs.ctypes.data, count, a.ctypes.data,
                                                               out.ctypes.data if want_out else None, int(flags),
                                                               mix.ctypes.data if want_mix else None))
        if out is None and mix is None:
            return None
        return self._callback_close(out, mix)

    def apply_material_fd(self, in_buffer, absorption, transmission, scattering):
        """UMaterialAcousticProcessor::ApplyMaterialFD (MAP.cpp:8-107) -> (specular, diffuse, transmitted)"""
        x = np.ascontiguousarray(in_buffer, dtype=np.float32).reshape(-1)
        a = np.ascontiguousarray(absorption, dtype=np.float32).reshape(-1)
        t = np.ascontiguousarray(transmission, dtype=np.float32).reshape(-1)
        sc = np.ascontiguousarray(scattering, dtype=np.float32).reshape(-1)
        if not (a.size == t.size == sc.size):
            raise _capi.FrequenSeeError(_capi.ERR_SIZE_MISMATCH, "response curves differ in length")
        outs = [np.zeros(x.size, dtype=np.float32) for _ in range(3)]
        self.check(self.lib.fs_apply_material_fd(self.h, x.ctypes.data, x.size, a.ctypes.data, t.ctypes.data,
                                                 sc.ctypes.data, a.size, *[o.ctypes.data for o in outs]))
        return tuple(outs)

    def set_profiling(self, level=2, interval=1):
        """0 off, 1 = HIP events around the dominant (walk) kernel only (every `interval`-th frame), 2 = every kernel,
        3 = 2 + the kernels count the records they fetch"""
        self.check(self.lib.fs_set_profiling(self.h, int(level)))
        self.check(self.lib.fs_set_profiling_interval(self.h, int(interval)))

    def stats(self):
        s = _capi.Stats()
        self.check(self.lib.fs_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self.check(self.lib.fs_reset_stats(self.h))

    def streams(self):
        """fs_get_streams: (compute stream, tail stream) as integer hipStream_t handles"""
        a, b = C.c_void_p(), C.c_void_p()
        self.check(self.lib.fs_get_streams(self.h, C.byref(a), C.byref(b)))
        return int(a.value or 0), int(b.value or 0)

    def pipeline_counters(self):
        """fs_get_pipeline_counters: the producer side's host counters since the context was created"""
        c = _capi.PipelineCounters()
        c.struct_size = C.sizeof(_capi.PipelineCounters)
        self.check(self.lib.fs_get_pipeline_counters(self.h, C.byref(c)))
        return c.as_dict()


class FrequenSeeAudioComponent:
    """UFrequenSeeAudioComponent's energy/IR surface (FSAC.h:69-91, 112-113, 133-143)."""

    def __init__(self, location=(0.0, 0.0, 0.0)):
        self._location = np.asarray(location, dtype=np.float32)
        self._subsys = None
        self._src = None
        self.bApplyReverb = True  # FSAC.h:60

    # OnRegister / OnUnregister (FSAC.cpp:42-64): auto-hook into the subsystem
    def OnRegister(self, subsystem: "AudioRayTracingSubsystem"):
        subsystem.RegisterSource(self)

    def OnUnregister(self):
        if self._subsys is not None:
            self._subsys.UnRegisterSource(self)

    def _ctx(self) -> Context:
        if self._subsys is None:
            raise RuntimeError("component is not registered with an AudioRayTracingSubsystem")
        return self._subsys.ctx

    @property
    def NumBins(self):
        return self._ctx().num_bins

    @property
    def NumSamples(self):
        return self._ctx().num_samples

    def GetComponentLocation(self):
        return self._location.copy()

    def SetComponentLocation(self, xyz):
        self._location = np.asarray(xyz, dtype=np.float32)
        if self._subsys is not None:
            self._ctx().set_source_position(self._src, self._location)

    def SetForwardVector(self, forward):
        """the owner's GetForwardVector(): what the directivity table is measured from"""
        self._ctx().set_source_orientation(self._src, forward)

    def SetDirectivity(self, gains=None):
        """per-band gains [bands][samples] over 0 .. 180 degrees from the forward vector; None = omnidirectional"""
        self._ctx().set_source_directivity(self._src, gains)

    def SetOrderWindow(self, min_order=0, max_order=None):
        """traced frames keep only the paths of min_order .. max_order hits (None: unbounded); (0, None) = everything.  With the
        direct renderer alone min_order = 1, with first-order voices too 2, with second-order voices too 3"""
        self._ctx().set_source_order_window(self._src, min_order, max_order)

    def GetOrderWindow(self):
        return self._ctx().source_order_window(self._src)

    @property
    def EnergyBuffer(self):
        """[NumBins] for one band (the reference), [bands][NumBins] otherwise"""
        e = self._ctx().energy_buffer(self._src)
        return e[0] if e.shape[0] == 1 else e

    def FlushEnergyBuffer(self):  # FSAC.h:76-79
        c = self._ctx()
        c.check(c.lib.fs_flush_energy_buffer(c.h, self._src))

    def UpdateEnergyBuffer(self, NewEnergyValues):  # FSAC.h:81-85 (check -> exception)
        c = self._ctx()
        v = np.ascontiguousarray(NewEnergyValues, dtype=np.float32)
        c.check(c.lib.fs_update_energy_buffer(c.h, self._src, v.ctypes.data, v.size))

    def AddEnergyAtDelay(self, DelaySeconds, EnergyValue, Band=0):  # FSAC.h:87-91
        c = self._ctx()
        c.check(c.lib.fs_add_energy_at_delay(c.h, self._src, Band, float(DelaySeconds), float(EnergyValue)))

    def ReconstructImpulseResponse(self, params=None):  # FSAC.cpp:320-380
        self._ctx().reconstruct_impulse_response(self._src, params)

    def GetImpulseResponse(self):  # FSAC.h:113 -> [NumChannels][NumSamples]
        c = self._ctx()
        return [c.impulse_response_view(self._src, ch) for ch in range(c.cfg.num_channels)]

    def SetImpulseResponse(self, ir):
        """write through the mutable reference GetImpulseResponse() returns (FSAC.h:113)"""
        self._ctx().set_impulse_response(self._src, ir)

    def GenerateDummyImpulseResponse(self):  # FSAC.cpp:408-452 as it ends up: a delta at samples 0 and N-1
        ir = np.zeros(self.NumSamples, np.float32)
        ir[0] = 1.0
        ir[-1] = 1.0
        self.SetImpulseResponse(ir)
        return ir

    def GetBandImpulseResponse(self, band):
        return self._ctx().band_impulse_response(self._src, band)

    def GetRoomParameters(self):
        """the room parameters published with the front IR (a reconstruct with FS_FLAG_ROOM_PARAMETERS): (sequence, [bands])"""
        return self._ctx().room_parameters(self._src)

    def GetDirectPath(self, **params):
        """not in the reference (its occlusion plugin is a no-op): this source's direct sound — one row of Context.direct_paths"""
        self._subsys._commit()
        return self._ctx().direct_paths([self._src], **params)[0]

    # legacy per-frame forward tracer (TickComponent -> UpdateSound, FSAC.cpp:103-109, 283-306)
    RaycastsPerTick = 1500      # FSAC.h:39
    RaycastBounces = 10         # FSAC.h:42
    RaycastDistance = 5000.0    # FSAC.h:45

    def UpdateSound(self, seed=0x5EED, listener_radius=34.0):
        self._subsys._commit()
        p = _capi.default_sound_params(raycasts_per_tick=self.RaycastsPerTick, raycast_bounces=self.RaycastBounces,
                                       raycast_distance=self.RaycastDistance, seed=seed,
                                       listener_radius=listener_radius)
        return self._ctx().update_sound(self._src, p)

    def GetOcclusionAttenuation(self):  # FSAC.h:112
        return self._ctx().occlusion_attenuation(self._src)


class AudioRayTracingSubsystem:
    """UAudioRayTracingSubsystem's registries and per-source update (ARTS.h:86-196, ARTS.cpp:45-195)."""

    USED_RAY_COUNT = 1000  # ARTS.h:176

    def __init__(self, num_bands=1, device=0, rank=0, world_size=1, stream=None, comm_id=None):
        """comm_id: the 128 bytes of Context.comm_unique_id() (made by rank 0, shipped to all ranks): the subsystem of
        a sharded run (world_size > 1) then sums every frame's energy buffer over the ranks inside the library"""
        self.ctx = Context(num_bands=num_bands, device=device, rank=rank, world_size=world_size, stream=stream)
        if comm_id is not None:
            self.ctx.comm_init(comm_id)
        self.ActiveSources = []
        self._geom = []          # registered (triangles, material_ids, actor ids)
        self._next_actor = 0
        self._materials = None
        self._dirty = True
        self._committed = False   # the first commit builds the tree on the host (SAH), later registration changes on the device
        self.params = _capi.default_params()

    def Deinitialize(self):
        self.ctx.close()

    # RegisterGeometry / UnregisterGeometry (ARTS.h:99-100): a "component" is a triangle set + material ids
    def RegisterGeometry(self, triangles, material_ids, object_ids=None):
        """one UAcousticGeometryComponent = one actor, unless per-triangle actor ids are given"""
        tri = np.asarray(triangles, dtype=np.float32).reshape(-1, 3, 3)
        if object_ids is None:
            obj = np.full(tri.shape[0], self._next_actor, dtype=np.uint32)
            self._next_actor += 1
        else:
            obj = np.asarray(object_ids, dtype=np.uint32).reshape(-1)
            self._next_actor = max(self._next_actor, int(obj.max(initial=0)) + 1)
        comp = (tri, np.asarray(material_ids, dtype=np.uint16).reshape(-1), obj)
        self._geom.append(comp)
        self._dirty = True
        return comp

    def UnregisterGeometry(self, comp):
        self._geom = [g for g in self._geom if g is not comp]
        self._dirty = True

    def SetMaterials(self, absorption, transmission=None, scattering=None):
        self._materials = (absorption, transmission, scattering)
        self._dirty = True

    def _commit(self):
        if not self._dirty:
            return
        if self._geom:
            tri = np.concatenate([g[0] for g in self._geom], axis=0)
            mat = np.concatenate([g[1] for g in self._geom], axis=0)
            obj = np.concatenate([g[2] for g in self._geom], axis=0)
        else:
            tri, mat, obj = np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.uint16), None
        ab, tr, sc = self._materials if self._materials is not None else (
            np.zeros((0, self.ctx.num_bands), np.float32), None, None)
        # the first commit builds the SAH tree on the host; a registration change during play takes the device-built tree at
        # once and gets the SAH tree swapped in when the library's background thread has built it
        self.ctx.set_scene(tri, mat, ab, tr, sc, object_ids=obj, fast="progressive" if self._committed else False)
        self._dirty = False
        self._committed = True

    def RebuildQuality(self):
        """after run-time registration changes (device-built Morton tree): the host's SAH build again, when a frame can afford it"""
        self._dirty, self._committed = True, False
        self._commit()

    def GeometryMoved(self, comp_index, triangles):
        """A registered geometry component (index in registration order) moved: same triangle count, new
        world-space positions.  Rewritten in place + device refit before the next trace (no rebuild)."""
        self._commit()
        first = sum(g[0].shape[0] for g in self._geom[:comp_index])
        tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3)
        if tri.shape[0] != self._geom[comp_index][0].shape[0]:
            raise ValueError("a moved component keeps its triangle count")
        self._geom[comp_index] = (tri, *self._geom[comp_index][1:])
        self.ctx.update_triangles(first, tri)

    def RegisterSource(self, InComp: FrequenSeeAudioComponent):  # ARTS.cpp:45-48
        InComp._subsys = self
        InComp._src = self.ctx.create_source(InComp._location)
        self.ActiveSources.append(InComp)

    def UnRegisterSource(self, InComp: FrequenSeeAudioComponent):  # ARTS.cpp:50-53
        if InComp in self.ActiveSources:
            self.ActiveSources.remove(InComp)
            self.ctx.destroy_source(InComp._src)
            InComp._subsys = None
            InComp._src = None

    def SetListenerLocation(self, xyz):  # PlayerPawn->GetActorLocation(), ARTS.cpp:287
        self.ctx.set_listener(xyz)

    def UpdateSource(self, Src: FrequenSeeAudioComponent, params=None):
        """ARTS.cpp:128-195: trace, evaluate, flush, deposit, reconstruct.  Returns the energy buffer."""
        self._commit()
        p = params or self.params
        e = self.ctx.compute_energy_response(Src._src, p)
        self.ctx.reconstruct_impulse_response(Src._src, p)
        return e

    def ForceUpdateSources(self):  # ARTS.cpp:883-886 — all active sources in one batched frame
        srcs = list(self.ActiveSources)
        if not srcs:
            return
        self._commit()
        self.ctx.update_sources([s._src for s in srcs], self.params)

    def _update_paths(self, kind, **params):
        """the body of the Update*Paths methods: Context.<kind>_paths over the active sources, PATH_QUERY[kind].max_batch at a time;
        without sources empty arrays — (rows [0], paths [0][0]), or rows [0] of an out-only query"""
        q = _capi.PATH_QUERY[kind]
        srcs = [s._src for s in self.ActiveSources]
        if not srcs:
            empty = np.zeros(0, dtype=record_dtype(q.path))
            return empty if q.row is None else (np.zeros(0, dtype=record_dtype(q.row)), empty.reshape(0, 0))
        self._commit()
        query = getattr(self.ctx, kind + "_paths")
        parts = [query(srcs[i:i + q.max_batch], **params) for i in range(0, len(srcs), q.max_batch)]
        if q.row is None:
            return np.concatenate(parts)
        return np.concatenate([r for r, _ in parts]), np.concatenate([p for _, p in parts])

    def UpdateDirectPaths(self, **params):
        """the direct sound of all active sources in one launch: a structured array, row i for ActiveSources[i]
        (Context.direct_paths; more than 256 sources take one launch per 256)"""
        return self._update_paths("direct", **params)

    def UpdateReflectionPaths(self, **params):
        """the first-order specular reflections of all active sources: (rows, paths), row i and paths[i] for ActiveSources[i]
        (Context.reflection_paths; more than 256 sources take one call per 256)"""
        return self._update_paths("reflection", **params)

    def UpdateDiffractionPaths(self, **params):
        """the first-order edge diffraction of all active sources: (rows, paths), row i and paths[i] for ActiveSources[i]
        (Context.diffraction_paths; more than 256 sources take one call per 256)"""
        return self._update_paths("diffraction", **params)

    def UpdateReflection2Paths(self, **params):
        """the second-order specular reflections of all active sources: (rows, paths), row i and paths[i] for ActiveSources[i]
        (Context.reflection2_paths; more than 256 sources take one call per 256)"""
        return self._update_paths("reflection2", **params)

    def UpdateDiffraction2Paths(self, **params):
        """the diffraction round thick obstacles of all active sources: (rows, paths), row i and paths[i] for ActiveSources[i]
        (Context.diffraction2_paths; more than 256 sources take one call per 256)"""
        return self._update_paths("diffraction2", **params)

    def UpdateMixedPaths(self, **params):
        """the paths off one reflector and round one edge of all active sources: (rows, paths), row i and paths[i] for
        ActiveSources[i] (Context.mixed_paths; more than 256 sources take one call per 256)"""
        return self._update_paths("mixed", **params)

    def SetPathingProbes(self, xyz=None, **bake_params):
        """the probe graph of the registered geometry: the probes (Context.pathing_set_probes) and, with any, the bake
        (Context.pathing_bake); returns the number of edges.  Bake again when a door has moved (PathingInfo()["scene_changed"])"""
        self.ctx.pathing_set_probes(xyz)
        if not self.ctx.pathing_info()["probes"]:
            return 0
        self._commit()
        return self.ctx.pathing_bake(**bake_params)

    def PathingInfo(self):
        return self.ctx.pathing_info()

    def UpdatePathingPaths(self, **params):
        """the route through the probe graph of all active sources: row i for ActiveSources[i] (Context.pathing_paths; more than
        256 sources take one call per 256)"""
        return self._update_paths("pathing", **params)

    def SetPipelining(self, depth):
        """fs_set_pipelining: Tick then updates the sources one after the other like the reference's loop (ARTS.cpp:60-68),
        streamed — every call launches one kernel that plans this source's frame, walks the previous source's and
        connects the one before — and ends with fs_submit; the IRs appear as they are published"""
        self.ctx.set_pipelining(depth)
        self._streamed = bool(depth)

    def SetFramesPerLaunch(self, n):
        """fs_set_frames_per_launch: the streamed sources of a Tick share launches n at a time (every source keeps its own
        seed, energy buffer and IR; Tick's closing fs_submit sends a partial group off)"""
        self.ctx.set_frames_per_launch(n)

    def Tick(self, DeltaTime):  # ARTS.cpp:55-85 without the 1 s warm-up: the caller drives every frame
        if not self.ActiveSources:
            return
        if getattr(self, "_streamed", False):
            self._commit()
            for s in self.ActiveSources:
                self.ctx.compute_energy_response_async(s._src, self.params)
                self.ctx.reconstruct_impulse_response_async(s._src, self.params)
            self.ctx.submit()
        else:
            self.ForceUpdateSources()
        # the reference draws from the engine's global rand() stream: every frame sees fresh samples
        self.params.seed = (self.params.seed + 1) & 0xFFFFFFFFFFFFFFFF

    def LineTraceSingle(self, start, end):
        """closest hit on the segment [start, end] (UWorld::LineTraceSingleByObjectType contract)"""
        self._commit()
        s, e = np.asarray(start, np.float32), np.asarray(end, np.float32)
        d = e - s
        ln = float(np.linalg.norm(d))
        if ln <= 0:
            return False, 0.0, -1, np.zeros(3, np.float32)
        hit, t, tri, n = self.ctx.trace_rays(s[None], (d / ln)[None], ln)
        return bool(hit[0]), float(t[0]), int(tri[0]), n[0]


class FrequenSeeAudioReverbPlugin:
    """FFrequenSeeAudioReverbPlugin (Private/FrequenSeeAudioReverbPlugin.h:46-47, .cpp:74-213): per audio
    callback, convolve the last IR-1 + BufferLength samples of a source with its impulse response."""

    def __init__(self, subsystem: AudioRayTracingSubsystem):
        self.ctx = subsystem.ctx
        self.FrameSize = 1024      # AudioCallbackBufferFrameSize, Config/DefaultEngine.ini:13
        self.Ears = False          # not in the reference: a two-ear late field (Context.reverb_ears_set installs the set first)

    def Initialize(self, BufferLength=1024):
        self.FrameSize = int(BufferLength)

    def OnInitSource(self, component: FrequenSeeAudioComponent):
        # Ears need the partitioned engine: both are the next init's.  Ears = False only takes the ears away: the engine stays
        # whatever SetEngine (or an earlier init with ears) chose — switch back with SetEngine(component, REVERB_ENGINE_DIRECT).
        if self.Ears:
            self.ctx.reverb_set_engine(component._src, _capi.REVERB_ENGINE_PARTITIONED)
        self.ctx.reverb_set_ears(component._src, self.Ears)
        self.ctx.reverb_init(component._src, self.FrameSize)

    def OnReleaseSource(self, component: FrequenSeeAudioComponent):
        self.ctx.reverb_release(component._src)

    def ProcessSourceAudio(self, component: FrequenSeeAudioComponent, AudioBuffer, literal_tail=False):
        return self.ctx.reverb_process(component._src, AudioBuffer, apply_reverb=component.bApplyReverb,
                                       literal_tail=literal_tail)

    def ProcessSourcesAudio(self, components, buffers, literal_tail=False, want_out=True, want_mix=False):
        """the mixer's loop over ProcessSourceAudio (RVB.cpp:118-170) as one call: buffers[i] is components[i]'s block; each
        component's bApplyReverb is honoured.  Returns what Context.reverb_process_batch does."""
        return self.ctx.reverb_process_batch([c._src for c in components], buffers, apply=[c.bApplyReverb for c in components],
                                             literal_tail=literal_tail, want_out=want_out, want_mix=want_mix)

    def SetCrossfade(self, component: FrequenSeeAudioComponent, samples):
        """not in the reference: fade each new impulse response in over `samples` output samples (0: abrupt switch)"""
        self.ctx.reverb_set_crossfade(component._src, samples)

    def SetEngine(self, component: FrequenSeeAudioComponent, engine):
        """not in the reference: the convolution engine of the source's next OnInitSource (_capi.REVERB_ENGINE_*)"""
        self.ctx.reverb_set_engine(component._src, engine)


class FrequenSeeAudioSoundfieldReverbPlugin(FrequenSeeAudioReverbPlugin):
    """Not in the reference: the reverb plugin with the late field on an ambisonic bus of (Order + 1)^2 channels, ACN order and SN3D
    normalisation (fs_reverb_soundfield_process_batch) — the diffuse counterpart of FrequenSeeAudioAmbisonicPlugin's voices, whose
    mix it is summed with.  SetOrder installs the context's carrier set; OnInitSource selects the partitioned engine and the
    soundfield.  The output is not clamped and bApplyReverb is not read: the call has no bypass row."""

    def __init__(self, subsystem: AudioRayTracingSubsystem):
        super().__init__(subsystem)
        self.Order = 1   # 0 .. MAX_AMBISONIC_ORDER; SetOrder before OnInitSource

    def SetOrder(self, Order=1):
        self.ctx.reverb_soundfield_set(int(Order))
        self.Order = int(Order)

    def OnInitSource(self, component: FrequenSeeAudioComponent):
        self.ctx.reverb_set_engine(component._src, _capi.REVERB_ENGINE_PARTITIONED)
        self.ctx.reverb_set_ears(component._src, False)
        self.ctx.reverb_set_soundfield(component._src, True)
        self.ctx.reverb_init(component._src, self.FrameSize)

    def ProcessAudio(self, components, buffers, want_out=True, want_mix=False):
        """buffers[i] is components[i]'s stereo block -> what Context.reverb_soundfield_process_batch returns"""
        return self.ctx.reverb_soundfield_process_batch([c._src for c in components], buffers, want_out=want_out, want_mix=want_mix)

    def ProcessSourceAudio(self, component: FrequenSeeAudioComponent, AudioBuffer, literal_tail=False):
        return self.ProcessAudio([component], [AudioBuffer])[0]

    def ProcessSourcesAudio(self, components, buffers, literal_tail=False, want_out=True, want_mix=False):
        return self.ProcessAudio(components, buffers, want_out=want_out, want_mix=want_mix)

    def ImpulseResponses(self, component: FrequenSeeAudioComponent):
        """h_c [C][num_samples] of the source's newest impulse response, for a host with a convolver of its own"""
        return self.ctx.reverb_soundfield_impulse_responses(component._src)


class FrequenSeeAudioOcclusionPlugin:
    """FFrequenSeeAudioOcclusionPlugin (Private/FrequenSeeAudioOcclusionPlugin.cpp:33-50), with the multiply the reference
    leaves commented out done: per audio callback every source's block is delayed by its direct path's arrival time and
    filtered by its per-band transmission.  Distance attenuation stays the host's."""

    def __init__(self, subsystem: AudioRayTracingSubsystem):
        self.ctx = subsystem.ctx
        self.FrameSize = 1024
        self.Taps = 255
        self.MaxDelaySeconds = 1.0

    def Initialize(self, BufferLength=1024, Taps=255, MaxDelaySeconds=1.0):
        self.FrameSize, self.Taps, self.MaxDelaySeconds = int(BufferLength), int(Taps), float(MaxDelaySeconds)

    def OnInitSource(self, component: FrequenSeeAudioComponent):
        self.ctx.direct_render_init(component._src, self.FrameSize, self.Taps, self.MaxDelaySeconds)

    def OnReleaseSource(self, component: FrequenSeeAudioComponent):
        self.ctx.direct_render_release(component._src)

    def Targets(self, paths):
        """the callback's targets from UpdateDirectPaths rows: band_gain = transmission, delay = the path's arrival time less
        the filter's own latency of (Taps - 1) / 2 samples, not below 0"""
        t = np.zeros(len(paths), dtype=Context.RENDER_TARGET_DTYPE)
        latency = ((self.Taps - 1) // 2) / float(self.ctx.cfg.sample_rate)
        for i, p in enumerate(paths):
            t[i]["delay"] = max(float(p["delay"]) - latency, 0.0)
            t[i]["band_gain"] = p["transmission"]
        return t

    def ProcessAudio(self, components, buffers, paths, want_out=True, want_mix=False):
        """buffers[i] is components[i]'s block, paths[i] its row of UpdateDirectPaths.  Returns what
        Context.direct_render_process_batch does."""
        return self.ctx.direct_render_process_batch([c._src for c in components], buffers, self.Targets(paths),
                                                    want_out=want_out, want_mix=want_mix)


class FrequenSeeAudioReflectionPlugin:
    """Not in the reference: per audio callback every source's block is rendered once per first-order reflection of
    UpdateReflectionPaths — delayed by the path's arrival time (fractional and slew-limited: each reflection has a Doppler shift of
    its own), filtered by its per-band reflectance, weighted by a per-channel gain and summed (fs_reflection_render_process_batch).
    A reflection is recognised from callback to callback by its triangle; one that appears or vanishes fades over one block.
    Panning and the distance law are this plugin's (Voices), not the library's."""

    def __init__(self, subsystem: AudioRayTracingSubsystem):
        self.ctx = subsystem.ctx
        self.FrameSize = 1024
        self.Taps = 255
        self.VoiceCount = 32
        self.MaxDelaySeconds = 1.0

    def Initialize(self, BufferLength=1024, Taps=255, Voices=32, MaxDelaySeconds=1.0):
        self.FrameSize, self.Taps, self.VoiceCount, self.MaxDelaySeconds = int(BufferLength), int(Taps), int(Voices), float(MaxDelaySeconds)

    def OnInitSource(self, component: FrequenSeeAudioComponent):
        self.ctx.reflection_render_init(component._src, self.FrameSize, self.Taps, self.VoiceCount, self.MaxDelaySeconds)

    def OnReleaseSource(self, component: FrequenSeeAudioComponent):
        self.ctx.reflection_render_release(component._src)

    @staticmethod
    def SecondOrderKey(a, b):
        """the key of the voice of a second-order path off the triangles a and b: 0x40000000 | (h >> 2) with
        h = (a * 2654435761 + b) mod 2^32 — no first-order key (a triangle below 2^29), no diffraction key (0x80000000 | ...)"""
        return _capi.REFLECTION2_VOICE_TAG | (((int(a) * 2654435761 + int(b)) & 0xFFFFFFFF) >> 2)

    @staticmethod
    def Diffraction2Key(triangle, edge):
        """the key of the voice of a path round the edge records (triangle[0], edge[0]) and (triangle[1], edge[1]):
        0x20000000 | (h >> 3) with h = ((4 i_p + j_p) * 2654435761 + (4 i_q + j_q)) mod 2^32 — the one range no other kind uses"""
        kp, kq = 4 * int(triangle[0]) + int(edge[0]), 4 * int(triangle[1]) + int(edge[1])
        return _capi.DIFFRACTION2_VOICE_TAG | (((kp * 2654435761 + kq) & 0xFFFFFFFF) >> 3)

    @staticmethod
    def MixedKey(triangle, edge, end):
        """the key of the voice of a path off the reflector triangle[0] and round the edge record (triangle[1], edge) with the
        reflector at `end`: 0xC0000000 | (h >> 2) with h = (m * 2654435761 + 4 (2 (4 i + j) + end)) mod 2^32 — above every first-order
        diffraction key (0x80000000 | (4 triangle + edge)) of a scene of fewer than 2^28 triangles"""
        return _capi.MIXED_VOICE_TAG | (((int(triangle[0]) * 2654435761 + 4 * (2 * (4 * int(triangle[1]) + int(edge)) + int(end))) & 0xFFFFFFFF) >> 2)

    def Voices(self, row, paths, right=None, reference_length=None, diffraction=None, second=None, diffraction2=None, mixed=None,
               pathing=None):
        """one source's entries from its UpdateReflectionPaths result (row: its counts, paths: its path array), over the first
        row["returned"] paths: key = triangle, band_gain = reflectance, delay = the path's arrival time less the filter's own
        latency of (Taps - 1) / 2 samples, not below 0.  channel_gain = (1, 1); with `right` (the listener's unit right vector) the
        constant-power pan (cos t, sin t), t = (dot(direction, right) + 1) pi / 4; with reference_length (cm) scaled by
        min(1, reference_length / length).  diffraction = (row, paths) of the same source from UpdateDiffractionPaths appends one
        voice per returned diffraction path — band_gain = gain, delay, pan and distance law as above, key = 0x80000000 |
        (4 triangle + edge): no reflection's key while the scene has fewer than 2^29 triangles, which is checked.  second = (row,
        paths) of the same source from UpdateReflection2Paths appends one voice per returned second-order path — band_gain =
        reflectance, delay, pan and distance law as above, key = SecondOrderKey(triangle[0], triangle[1]).  Two second-order paths
        of the row whose keys collide: the earlier in the row — the shorter, ties by (a, b) — is kept and the other dropped (the
        renderer refuses duplicate keys).  diffraction2 = (row, paths) of the same source from UpdateDiffraction2Paths appends, last,
        one voice per returned path round two edges — band_gain = gain, key = Diffraction2Key(triangle, edge); on colliding keys
        the earlier in the row is kept likewise.  mixed = (row, paths) of the same source from UpdateMixedPaths appends, after
        those, one voice per returned path off a reflector and round an edge — band_gain = gain, key = MixedKey(triangle, edge,
        end), colliding keys likewise; with it a diffraction path's triangle must stay below 2^28, which is checked.  pathing = the
        source's row of UpdatePathingPaths appends, last, one voice if the row is FOUND and not DIRECT — band_gain = gain, delay,
        pan (from `direction`, towards the first probe) and distance law as for a diffraction path, key = PATHING_VOICE_KEY
        (0x80000003: no diffraction key, whose low bits are an edge 0 .. 2)."""
        entries = self._path_entries(row, paths, diffraction, second, diffraction2, mixed, pathing)
        v = np.zeros(len(entries), dtype=Context.REFLECTION_VOICE_DTYPE)
        latency = ((self.Taps - 1) // 2) / float(self.ctx.cfg.sample_rate)
        r = None if right is None else np.asarray(right, np.float64).reshape(3)
        for o, (key, p, band_gain) in zip(v, entries):
            o["key"] = key
            o["delay"] = max(float(p["delay"]) - latency, 0.0)
            o["band_gain"] = band_gain
            left_right = np.ones(2, np.float64)
            if r is not None:
                t = (float(np.dot(np.asarray(p["direction"], np.float64), r)) + 1.0) * np.pi / 4.0
                left_right = np.array([np.cos(t), np.sin(t)])
            if reference_length is not None:
                left_right = left_right * min(1.0, float(reference_length) / float(p["length"]))
            o["channel_gain"] = left_right
        return v

    # The kinds of path Voices() walks, in its order: (name, key of a path record, band-gain field, are colliding keys dropped).
    # The pathing voice, one record and no list, comes after them.
    _KINDS = (
        ("reflection", lambda self, p: int(p["triangle"]), "reflectance", False),
        ("diffraction", lambda self, p: _capi.DIFFRACTION_VOICE_TAG | (int(p["triangle"]) * 4 + int(p["edge"])), "gain", False),
        ("second", lambda self, p: self.SecondOrderKey(p["triangle"][0], p["triangle"][1]), "reflectance", True),
        ("diffraction2", lambda self, p: self.Diffraction2Key(p["triangle"], p["edge"]), "gain", True),
        ("mixed", lambda self, p: self.MixedKey(p["triangle"], p["edge"], p["end"]), "gain", True),
    )
    # The range checks, in the order they are made on a path: (the kinds whose triangle is checked, the kinds whose presence arms
    # the check, the limit, the error)
    _RANGE_CHECKS = (
        (("reflection", "diffraction"), ("diffraction", "second", "diffraction2", "mixed"), _capi.REFLECTION2_VOICE_TAG >> 1,
         "Voices: triangle index 2^29 or above: the keys of the path kinds would collide"),
        (("diffraction",), ("mixed",), _capi.MIXED_VOICE_TAG >> 4,
         "Voices: a diffraction path's triangle index is 2^28 or above: its key would collide with the mixed paths' keys"),
    )

    def _path_entries(self, row, paths, diffraction=None, second=None, diffraction2=None, mixed=None, pathing=None):
        """what Voices() keeps of a source's path records, in its order, as (key, path record, band gains): the keys, their range
        checks and the dropping of colliding keys as Voices() documents them"""
        given = dict(reflection=(row, paths), diffraction=diffraction, second=second, diffraction2=diffraction2, mixed=mixed)
        seen, kept = set(), []
        for name, key_of, gain_field, drop_collisions in self._KINDS:
            if given[name] is None:
                continue
            k_row, k_paths = given[name]
            checks = [(limit, text) for kinds, armed_by, limit, text in self._RANGE_CHECKS
                      if name in kinds and any(given[a] is not None for a in armed_by)]
            for p in k_paths[:int(k_row["returned"])]:
                for limit, text in checks:
                    if int(p["triangle"]) >= limit:
                        raise ValueError(text)
                key = key_of(self, p)
                if drop_collisions:
                    if key in seen:
                        continue
                    seen.add(key)
                kept.append((key, p, p[gain_field]))
        if pathing is not None and int(pathing["flags"]) & (_capi.PATHING_FOUND | _capi.PATHING_DIRECT) == _capi.PATHING_FOUND:
            kept.append((_capi.PATHING_VOICE_KEY, pathing, pathing["gain"]))
        return kept

    @staticmethod
    def _pick(i, diffraction, second, diffraction2, mixed, pathing):
        """source i's share of the optional path kinds ProcessAudio takes, as the keywords Voices() takes"""
        def pair(x):
            return None if x is None else (x[0][i], x[1][i])
        return dict(diffraction=pair(diffraction), second=pair(second), diffraction2=pair(diffraction2), mixed=pair(mixed),
                    pathing=None if pathing is None else pathing[i])

    def ProcessAudio(self, components, buffers, rows, paths, right=None, reference_length=None, want_out=True, want_mix=False,
                     diffraction=None, second=None, diffraction2=None, mixed=None, pathing=None):
        """buffers[i] is components[i]'s block, rows[i] / paths[i] its results of UpdateReflectionPaths; diffraction = the (rows,
        paths) of UpdateDiffractionPaths, second = the (rows, paths) of UpdateReflection2Paths, diffraction2 = the (rows, paths) of
        UpdateDiffraction2Paths, mixed = the (rows, paths) of UpdateMixedPaths, pathing = the rows of UpdatePathingPaths, or None.
        Returns what Context.reflection_render_process_batch does."""
        voices = [self.Voices(rows[i], paths[i], right, reference_length, **self._pick(i, diffraction, second, diffraction2, mixed, pathing))
                  for i in range(len(components))]
        return self.ctx.reflection_render_process_batch([c._src for c in components], buffers, voices,
                                                        want_out=want_out, want_mix=want_mix)


class FrequenSeeAudioBinauralPlugin(FrequenSeeAudioReflectionPlugin):
    """Not in the reference: the reflection plugin with every voice rendered from its arrival direction through a head-related
    impulse response set (fs_binaural_render_process_batch) instead of a pan: interaural delay and head shadow come out of the
    set.  The direct sound becomes a voice of the same call.  The listener's orientation (forward, right) is the host's, and so
    is any measured HRIR set (SetHrtf); without one SetHrtf() installs the library's spherical-head model."""

    DirectKey = _capi.BINAURAL_DIRECT_KEY   # a first-order key (a triangle index) no scene of fewer than 2^29 - 1 triangles uses

    def SetHrtf(self, dirs=None, hrir=None, directions=1024, taps=128, interpolate=False, align=False, onsets=None):
        """the context's HRIR set: dirs [n][3] (head frame: x forward, y right, z up) and hrir [n][2][H], or the spherical-head
        model of `directions` and `taps`.  interpolate: triangulate the set and install the mesh (fs_hrtf_set_mesh) — every
        voice's HRIR is then the blend of the three round its direction, not the nearest one.  align: carry the HRIRs' onsets
        apart (fs_hrtf_set_onsets), so that the blend is of aligned HRIRs and of their delays — `onsets` [n][2] where the host
        has them (hrir is then the aligned set), else split off the set given (fs_hrtf_split_onsets: threshold 0.1, lead 0);
        without a set, the spherical head with its two halves apart.  Before OnInitSource; not concurrent with ProcessAudio"""
        if onsets is not None and (not align or dirs is None):
            raise ValueError("onsets go with align=True and a host set: they are the delays of its aligned HRIRs")
        if onsets is not None and np.shape(onsets) != (np.shape(dirs)[0], 2):
            raise ValueError("onsets must be [n][2] for the n directions of the set")
        if dirs is None:
            if align:
                dirs, hrir, onsets = Context.hrtf_spherical_head_split(self.ctx.cfg.sample_rate, directions, taps)
            else:
                dirs, hrir = Context.hrtf_spherical_head(self.ctx.cfg.sample_rate, directions, taps)
        elif align and onsets is None:
            hrir, onsets = Context.hrtf_split_onsets(hrir, 0.1, 0)
        self.ctx.hrtf_set(dirs, hrir)
        if interpolate:
            self.ctx.hrtf_set_mesh(Context.hrtf_triangulate(dirs))
        if align:
            self.ctx.hrtf_set_onsets(onsets)

    def OnInitSource(self, component: FrequenSeeAudioComponent):
        self.ctx.binaural_render_init(component._src, self.FrameSize, self.Taps, self.VoiceCount, self.MaxDelaySeconds)

    def OnReleaseSource(self, component: FrequenSeeAudioComponent):
        self.ctx.binaural_render_release(component._src)

    def Voices(self, row, paths, forward, right, reference_length=None, direct=None, diffraction=None, second=None, diffraction2=None,
               mixed=None, pathing=None):
        """one source's entries: keys, delays (less the band filter's latency of (Taps - 1) / 2 samples, not below 0) and band
        gains exactly as FrequenSeeAudioReflectionPlugin.Voices builds them, from the same arguments; gain = min(1,
        reference_length / length) with reference_length (cm), else 1; direction = the path's arrival direction d in the head
        frame, (d . forward, d . right, d . up) with up = (f.y r.z - f.z r.y, f.z r.x - f.x r.z, f.x r.y - f.y r.x) — for forward
        = +x and right = +y that is up = +z.  direct = (the source's row of UpdateDirectPaths, the vector from the listener to the
        source in world space, any length but zero) puts the direct sound in front as one more voice: key = DirectKey (0x1FFFFFFF:
        a triangle index no scene of fewer than 2^29 - 1 triangles has, which is checked against the first-order keys), band_gain =
        transmission, length = distance.  pathing = the source's row of UpdatePathingPaths: one more voice, as the reflection plugin
        appends it, heard from the row's `direction`."""
        f = np.asarray(forward, np.float64).reshape(3)
        r = np.asarray(right, np.float64).reshape(3)
        up = np.array([f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]])
        latency = ((self.Taps - 1) // 2) / float(self.ctx.cfg.sample_rate)
        entries = []   # (key, delay, band gains, length, world direction)
        if direct is not None:
            d_row, to_source = direct
            entries.append((self.DirectKey, d_row["delay"], d_row["transmission"], d_row["distance"], to_source))
        for key, p, band_gain in self._path_entries(row, paths, diffraction, second, diffraction2, mixed, pathing):
            if direct is not None and key == self.DirectKey:
                raise ValueError("Voices: triangle index 2^29 - 1: its key is the direct sound's")
            entries.append((key, p["delay"], band_gain, p["length"], p["direction"]))
        v = np.zeros(len(entries), dtype=Context.BINAURAL_VOICE_DTYPE)
        for o, (key, delay, band_gain, length, d) in zip(v, entries):
            d = np.asarray(d, np.float64).reshape(3)
            o["key"] = key
            o["delay"] = max(float(delay) - latency, 0.0)
            o["band_gain"] = band_gain
            o["gain"] = 1.0 if reference_length is None else min(1.0, float(reference_length) / float(length))
            o["direction"] = [np.dot(d, f), np.dot(d, r), np.dot(d, up)]
        return v

    def ProcessAudio(self, components, buffers, rows, paths, forward, right, reference_length=None, want_out=True, want_mix=False,
                     direct=None, diffraction=None, second=None, diffraction2=None, mixed=None, pathing=None):
        """buffers[i] is components[i]'s block, rows[i] / paths[i] its results of UpdateReflectionPaths; direct = (the rows of
        UpdateDirectPaths, the listener's location) or None; the other path kinds as FrequenSeeAudioReflectionPlugin.ProcessAudio
        takes them.  Returns what Context.binaural_render_process_batch does."""
        voices = []
        for i, c in enumerate(components):
            d = None if direct is None else (direct[0][i], np.asarray(c.GetComponentLocation(), np.float64) - np.asarray(direct[1], np.float64))
            voices.append(self.Voices(rows[i], paths[i], forward, right, reference_length, d,
                                      **self._pick(i, diffraction, second, diffraction2, mixed, pathing)))
        return self._render(components, buffers, voices, want_out, want_mix)

    def _render(self, components, buffers, voices, want_out, want_mix):
        return self.ctx.binaural_render_process_batch([c._src for c in components], buffers, voices, want_out=want_out, want_mix=want_mix)


class FrequenSeeAudioAmbisonicPlugin(FrequenSeeAudioBinauralPlugin):
    """Not in the reference: the binaural plugin's voices — the same entries, Voices() unchanged — rendered into an ambisonic bus
    of (Order + 1)^2 channels, ACN order and SN3D normalisation (fs_ambisonic_render_process_batch), instead of two ears: for
    loudspeakers, for an engine's soundfield submix, for a host's own binaural decoder.  No HRIR set is needed.  Rotation (the bus
    is rendered in the head frame given to Voices(); a head tracker may rotate it later) and decoding are the host's."""

    Order = 1

    def OnInitSource(self, component: FrequenSeeAudioComponent):
        self.ctx.ambisonic_render_init(component._src, self.FrameSize, self.Taps, self.VoiceCount, self.MaxDelaySeconds, self.Order)

    def OnReleaseSource(self, component: FrequenSeeAudioComponent):
        self.ctx.ambisonic_render_release(component._src)

    def _render(self, components, buffers, voices, want_out, want_mix):
        """ProcessAudio is the binaural plugin's; returns what Context.ambisonic_render_process_batch does"""
        return self.ctx.ambisonic_render_process_batch([c._src for c in components], buffers, voices, want_out=want_out, want_mix=want_mix)


class MaterialAcousticProcessor:
    """Mirror of UMaterialAcousticProcessor (Public/MaterialAcousticProcessor.h:55-70).  Props is any object
    with Absorption / Transmission / Scattering response arrays (FMaterialAcousticFD, .h:24-37) or a 3-tuple."""

    def __init__(self, subsystem: AudioRayTracingSubsystem):
        self.subsystem = subsystem

    def ApplyMaterialFD(self, InBuffer, Props):
        if isinstance(Props, (tuple, list)):
            a, t, s = Props
        else:
            a, t, s = Props.Absorption, Props.Transmission, Props.Scattering
        spec, diff, trans = self.subsystem.ctx.apply_material_fd(InBuffer, a, t, s)
        return {"Specular": spec, "Diffuse": diff, "Transmitted": trans}   # FAcousticOutputs (.h:40-53)
