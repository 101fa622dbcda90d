"""What every path query (the rows of _capi.PATH_QUERIES) promises besides its own geometry, written once: the exported names and
their tier, the refusals without a device and on one, state left untouched, a steady state that allocates nothing, queries
interleaved on one context, and the batch, permuted-list and moved-actor checks.  tests/test_<kind>_paths.py describes its query
by a Query and calls these from tests of the same names; what differs between two queries in substance is a field of Query.
"""
import ctypes as C
import dataclasses
import os
from typing import Callable, Optional, Sequence

import numpy as np

DIRECT_SPHERE = dict(samples=16, source_radius=30.0)   # the direct query wherever it runs beside another one


@dataclasses.dataclass
class Query:
    kind: str                          # the row of _capi.PATH_QUERIES: the C functions, the records, the defaults, Context.<kind>_paths
    dtypes: Sequence[str]              # Context's names of the row and path dtypes (an out-only query: of its one record)
    world: Callable                    # () -> the World of the refusal and steady-state tests
    src: Sequence[float]               # the source there ...
    lis: Sequence[float]               # ... and the listener
    wrong_struct_size: int             # a struct_size the params do not have
    refused: Sequence[dict]            # keyword sets fs_update_<kind>_paths refuses on a device
    refused_without_device: Sequence[dict] = ()    # those the no-device test tries
    reach: dict = dataclasses.field(default_factory=dict)       # legal keywords with which src has paths: every refusal-test call carries them
    sentinel_paths: int = 16           # paths per row of the refusal test's buffers (the largest legal max_paths)
    null_paths: int = 8                # ... and of the no-device test's
    legal: Sequence[dict] = ()         # extreme but legal keyword sets: taken
    defaults_found: Optional[Callable] = None    # (t, oracle_mod, want): what ctx.<kind>_paths([src, src]) must have found
    legal_found: Optional[Callable] = None       # (rows): what the last of `legal` must have left in the first buffer
    untouched: dict = dataclasses.field(default_factory=dict)   # keywords of the call that must leave the sources alone
    untouched_found: Optional[Callable] = None   # (result): what that call must have found
    yardstick: Optional[Callable] = None         # (oracle_mod, world) -> the restatement, for ...
    empty_world: Optional[Callable] = None       # ... the empty committed scene
    steady: dict = dataclasses.field(default_factory=dict)      # keywords of the steady-state calls
    fewer: dict = dataclasses.field(default_factory=dict)       # those added for the call with 7 of the 40 sources: larger caps
    fewer_differs_in: Sequence[str] = ()         # row fields the larger caps change; the rest, and the paths both hold, are equal
    steady_found: Optional[Callable] = None      # (ctx, handles, first, fewer): what else the steady state must show

    def method(self, ctx):
        return getattr(ctx, self.kind + "_paths")

    def buffers(self, pkg, count, paths_per_row):
        """[rows [count], paths [count][paths_per_row]], or [rows [count]] of an out-only query, every byte 7"""
        shapes = [(count,), (count, paths_per_row)][:len(self.dtypes)]
        return [np.full(shape, 7, dtype=getattr(pkg.Context, name)) for shape, name in zip(shapes, self.dtypes)]


def as_tuple(result):
    return result if isinstance(result, tuple) else (result,)


def same_bytes(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def pointers(bufs):
    return [None if b is None else b.ctypes.data for b in bufs]


def place(ctx, positions):
    return [ctx.create_source(p) for p in positions]


def device_free_bytes():
    """hipMemGetInfo of the HIP runtime the library itself runs on (the copy of libamdhip64 already mapped into this process: a
    second runtime, such as the one torch brings along, finds no device once this one holds it)"""
    import sys
    torch_dir = os.path.dirname(sys.modules["torch"].__file__) if "torch" in sys.modules else None
    paths = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line]
    path = next(p for p in paths if torch_dir is None or not p.startswith(torch_dir))
    hip = C.CDLL(path)
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def assert_equal(got, want, where=""):
    """(rows, paths) of a rows-and-paths query against the restatement's: every field of every row and path, floats by bit pattern"""
    (grows, gpaths), (wrows, wpaths) = got, want
    assert grows.shape == wrows.shape and gpaths.shape == wpaths.shape, where
    for i in range(len(wrows)):
        for k in wrows.dtype.names:
            assert grows[i][k] == wrows[i][k], f"{where} row {i}: {k}: got {grows[i][k]!r}, restatement {wrows[i][k]!r}"
        for j in range(wpaths.shape[1]):
            for k in wpaths.dtype.names:
                g, x = np.atleast_1d(gpaths[i, j][k]), np.atleast_1d(wpaths[i, j][k])
                assert g.tobytes() == x.tobytes(), f"{where} row {i} path {j}: {k}: got {g!r}, restatement {x!r}"
    assert grows.tobytes() == wrows.tobytes() and gpaths.tobytes() == wpaths.tobytes(), where


def checker(kind):
    """check(pkg, ctx, y, handles, positions, listener, where, src_obj=None, lis_obj=NO_OBJECT, **params): ctx.<kind>_paths against
    the restatement y; -> what the call returned"""
    def check(pkg, ctx, y, handles, positions, listener, where, src_obj=None, lis_obj=0xFFFFFFFF, **params):
        got = getattr(ctx, kind + "_paths")(handles, **params)
        assert_equal(got, y.expect(pkg, positions, listener, src_obj, lis_obj, **params), where)
        return got
    return check


def transformed(w, actor, m):
    """w.tri with the triangles of `actor` at the row-major 3 x 4 matrix m, in fs_scene_set_object_transforms' order of operations"""
    moved = w.tri.copy()
    idx = w.obj == actor
    p = moved[idx]
    moved[idx] = np.stack([((m[k, 0] * p[..., 0] + m[k, 1] * p[..., 1]) + m[k, 2] * p[..., 2]) + m[k, 3] for k in range(3)], axis=-1)
    return moved


def exported_in_one_tier(pkg, names):
    cap = pkg._capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frequensee.h")).read()
    opening = header[:header.index("#ifndef FREQUENSEE_H")]
    core = opening[opening.index("CORE:"):opening.index("EXTENDED =")]
    extended = opening[opening.index("EXTENDED:"):]
    for name in names:
        assert name in cap.EXPORTS and hasattr(cap.load(), name)
        assert name in extended.split() and name not in core.split()
        assert opening.split().count(name) == 1
    return extended


def null_context_and_no_device(pkg, q):
    cap = pkg._capi
    lib = cap.load()
    table = cap.PATH_QUERY[q.kind]
    update = getattr(lib, table.update)
    src = (C.c_int32 * 1)(0)
    bufs = q.buffers(pkg, 1, q.null_paths)
    before = [b.tobytes() for b in bufs]
    ptrs = pointers(bufs)
    assert update(None, src, 1, None, *ptrs) == cap.ERR_INVALID_ARGUMENT
    getattr(lib, table.default)(None)   # tolerated, like the other *_default calls
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        cfg = cap.default_config(num_bands=1)
        assert lib.fs_context_create(C.byref(cfg), C.byref(h)) == cap.ERR_NO_DEVICE and h
        try:
            assert update(h, src, 1, None, *ptrs) == cap.ERR_NO_DEVICE
            assert b"no CPU fallback" in lib.fs_last_error(h)
            assert update(h, None, 1, None, *ptrs) == cap.ERR_INVALID_ARGUMENT
            for i in range(len(ptrs)):
                assert update(h, src, 1, None, *[None if j == i else p for j, p in enumerate(ptrs)]) == cap.ERR_INVALID_ARGUMENT, q.dtypes[i]
            for count in (0, 257):
                assert update(h, src, count, None, *ptrs) == cap.ERR_INVALID_ARGUMENT, count
            for kw in q.refused_without_device:
                p = cap.default_path_params(q.kind, **kw)
                assert update(h, src, 1, C.byref(p), *ptrs) == cap.ERR_INVALID_ARGUMENT, kw
        finally:
            lib.fs_context_destroy(h)
    assert [b.tobytes() for b in bufs] == before


_LISTED = object()   # Calls(): the source listed twice (None is a NULL pointer)


class Calls:
    """a context with one source listed twice, buffers for two rows with every byte 7, and fs_update_<kind>_paths on them"""

    def __init__(self, pkg, q):
        self.pkg, self.q, self.cap = pkg, q, pkg._capi
        self.update = getattr(self.cap.load(), self.cap.PATH_QUERY[q.kind].update)
        self.w = q.world()
        self.ctx = pkg.Context(num_bands=4)
        self.src = self.ctx.create_source(q.src)
        self.arr = (C.c_int32 * 2)(self.src, self.src)
        self.bufs = q.buffers(pkg, 2, q.sentinel_paths)
        self.sentinel = [b.tobytes() for b in self.bufs]

    def __call__(self, sources=_LISTED, count=2, params=None, dest=None, **kw):
        p = self.cap.default_path_params(self.q.kind, **dict(self.q.reach, **kw)) if (kw or params is None) else params
        return self.update(self.ctx.h, self.arr if sources is _LISTED else sources, count, C.byref(p), *pointers(self.bufs if dest is None else dest))

    def commit(self, ctx=None):
        w, ctx = self.w, ctx or self.ctx
        ctx.set_scene(w.tri, w.mat, w.absorption, w.transmission, getattr(w, "scattering", None), object_ids=w.obj)
        ctx.set_listener(self.q.lis)

    def unwritten(self):
        assert [b.tobytes() for b in self.bufs] == self.sentinel, "a refused call wrote"

    def refusals(self):
        """every refusal of the committed context, none of which writes"""
        cap, q, src = self.cap, self.q, self.src
        assert self(sources=None) == cap.ERR_INVALID_ARGUMENT
        for i in range(len(self.bufs)):
            assert self(dest=[None if j == i else b for j, b in enumerate(self.bufs)]) == cap.ERR_INVALID_ARGUMENT, q.dtypes[i]
        assert self.update(None, self.arr, 2, None, *pointers(self.bufs)) == cap.ERR_INVALID_ARGUMENT
        many = (C.c_int32 * 257)(*([src] * 257))
        big = q.buffers(self.pkg, 257, q.sentinel_paths)
        for bad in (0, -1, 257):
            assert self(sources=many, count=bad, dest=big) == cap.ERR_INVALID_ARGUMENT, bad
        assert same_bytes(big, q.buffers(self.pkg, 257, q.sentinel_paths))
        p = cap.default_path_params(q.kind)
        p.struct_size = q.wrong_struct_size
        assert self(params=p) == cap.ERR_INVALID_ARGUMENT
        for kw in q.refused:
            assert self(**kw) == cap.ERR_INVALID_ARGUMENT, kw
        assert self(sources=(C.c_int32 * 2)(src, 12345)) == cap.ERR_BAD_HANDLE
        assert self(sources=(C.c_int32 * 2)(-1, src)) == cap.ERR_BAD_HANDLE
        self.unwritten()

    def null_params_are_the_defaults(self):
        """-> what ctx.<kind>_paths([src, src]) returns, which a call with NULL params has been held to"""
        cap, q = self.cap, self.q
        bufs = q.buffers(self.pkg, 2, max(int(getattr(cap.default_path_params(q.kind), "max_paths", 0)), 0))
        assert self.update(self.ctx.h, self.arr, 2, None, *pointers(bufs)) == cap.OK
        want = as_tuple(q.method(self.ctx)([self.src, self.src]))
        assert same_bytes(bufs, want)
        return want


def leaves_sources_alone(pkg, ctx, src, query):
    """query(), a successful call, leaves the sources alone: energy, IR publish number, occlusion scalar"""
    fp = pkg.default_params(num_rays=512, depth=4, seed=3)
    ctx.compute_energy_response(src, fp)
    ctx.reconstruct_impulse_response(src, fp)
    ctx.update_sound(src, pkg._capi.default_sound_params(raycasts_per_tick=64))
    before = (ctx.energy_buffer(src).tobytes(), ctx.impulse_response_sequence(src), ctx.occlusion_attenuation(src), ctx.impulse_response(src).tobytes())
    query()
    after = (ctx.energy_buffer(src).tobytes(), ctx.impulse_response_sequence(src), ctx.occlusion_attenuation(src), ctx.impulse_response(src).tobytes())
    assert before == after


def errors_and_untouched_state(pkg, oracle_mod, q):
    t = Calls(pkg, q)
    cap, ctx = t.cap, t.ctx
    assert t() == cap.ERR_NOT_COMMITTED
    t.commit()
    t.refusals()
    # NULL params = the defaults; extreme but legal values are taken
    want = t.null_params_are_the_defaults()
    if q.defaults_found is not None:
        q.defaults_found(t, oracle_mod, want)
    for kw in q.legal:
        assert t(**kw) == cap.OK, kw
    if q.legal_found is not None:
        q.legal_found(t.bufs[0])

    def query():
        got = q.method(ctx)([t.src], **q.untouched)
        if q.untouched_found is not None:
            q.untouched_found(got)

    leaves_sources_alone(pkg, ctx, t.src, query)
    ctx.close()
    if q.empty_world is not None:   # an empty committed scene: rows of zeros
        e = q.empty_world()
        ctx = e.context(pkg)
        ctx.set_listener(q.lis)
        rows, paths = checker(q.kind)(pkg, ctx, q.yardstick(oracle_mod, e), place(ctx, [q.src, q.lis]), [q.src, q.lis], q.lis, "empty", **q.reach)
        assert np.all(rows.view(np.uint8) == 0) and np.all(paths.view(np.uint8) == 0)
        ctx.close()


def steady_state_allocates_nothing(pkg, q, opened=None, churn=None, found=None):
    """opened: (ctx, 40 handles) where the query's world and 40 sources at q.src will not do; churn(ctx): more work that must
    allocate nothing; found: q.steady_found where that needs what the test holds"""
    if opened is None:
        ctx = q.world().context(pkg)
        ctx.set_listener(q.lis)
        opened = ctx, place(ctx, [q.src] * 40)
    ctx, h = opened
    query = q.method(ctx)
    first = as_tuple(query(h, **q.steady))
    free0 = device_free_bytes()
    for _ in range(20):
        again = as_tuple(query(h, **q.steady))
    fewer = as_tuple(query(h[:7], **dict(q.steady, **q.fewer)))   # a smaller count, larger caps: fits what is there
    if churn is not None:
        churn(ctx)
    assert device_free_bytes() >= free0
    assert same_bytes(again, first)
    if q.fewer_differs_in:
        assert all(np.array_equal(fewer[0][k], first[0][k][:7]) for k in first[0].dtype.names if k not in q.fewer_differs_in)
    else:
        assert fewer[0].tobytes() == first[0][:7].tobytes()
    if len(first) > 1:
        assert fewer[1][:, :first[1].shape[1]].tobytes() == first[1][:7].tobytes()
    if (found or q.steady_found) is not None:
        (found or q.steady_found)(ctx, h, first, fewer)
    ctx.close()


def queries_interleaved_on_one_context(fresh, calls, params):
    """fresh() -> (a new context, its handles); calls: (kind, count) in order; params: kind -> keywords.  Each call on the one
    context returns the bytes it returns as the first call of a fresh context.  -> what the calls on the one context returned"""
    params = dict(dict(direct=DIRECT_SPHERE), **params)

    def run(ctx, h, kind, count):
        return as_tuple(getattr(ctx, kind + "_paths")(h[:count], **params.get(kind, {})))

    ctx, h = fresh()
    got = [run(ctx, h, kind, count) for kind, count in calls]
    ctx.close()
    first = {}
    for i, ((kind, count), g) in enumerate(zip(calls, got)):
        if (kind, count) not in first:
            one, h1 = fresh()
            first[kind, count] = run(one, h1, kind, count)
            one.close()
        want = first[kind, count]
        assert len(g) == len(want) and all(len(a) == count for a in g)
        for a, b in zip(g, want):
            assert a.tobytes() == b.tobytes(), f"call {i} ({kind}, count {count}) differs from the same call on a fresh context"
    return got


def batch_agrees(query, h, got, singles, **params):
    """rows, paths = got = query(h, **params) against the same sources one call each (singles), in a permuted list, and the first
    five alone (one confirm workgroup with idle waves beside a full one)"""
    rows, paths = got
    n = len(h)
    if singles:
        ones = [query([x], **params) for x in h]
        assert np.concatenate([r for r, _ in ones]).tobytes() == rows.tobytes(), f"count = {n} differs from {n} calls with count = 1"
        assert np.concatenate([p for _, p in ones]).tobytes() == paths.tobytes(), f"count = {n} differs from {n} calls with count = 1"
    perm = np.random.default_rng(7).permutation(n)
    prows, ppaths = query([h[i] for i in perm], **params)
    assert prows.tobytes() == rows[perm].tobytes() and ppaths.tobytes() == paths[perm].tobytes(), "a permuted list"
    frows, fpaths = query(h[:5], **params)
    assert frows.tobytes() == rows[:5].tobytes() and fpaths.tobytes() == paths[:5].tobytes()
