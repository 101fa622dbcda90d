"""Structural checker of the committed tree (not a test file; tests/test_tree_structure.py drives it).

Every array the tree kernels write (fs_build.hip: collapse_kernel, records_kernel; fs_refit.hip: update_tris_kernel,
pack_tris_kernel, refit_level_kernel, coop_nodes_kernel, coop16_kernel) is compared here with a plain numpy restatement
of the same operation, in float64 or in exact integers on bit patterns: no GPU, no oracle.  Every check returns a list of
findings, strings that begin with a code ("topology.child_level: ..."); an empty list means the arrays are right.

  a  check_topology   levels, links, leaf ranges, the permutation, the traversal-stack bound
  b  check_records    Tri48 / normals against Tri64, Tri64 against the inputs and against a host commit's records
  c  check_boxes      conservative AND tight quantised boxes, for any committed tree
  d  check_refit      refit_level_kernel restated exactly (device builds, any tree after fs_scene_refit)
  e  check_coop4      coop_nodes_kernel restated exactly
  f  check_coop16     coop16_kernel restated exactly
"""
import ctypes as C

import numpy as np

# ---- the five records (audio-pathtracer_amd/csrc/fs_internal.hpp) ---------------------------------------------------------
NODE_DT = np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("sx", "<f4"),
                    ("lox", "<u4"), ("loy", "<u4"), ("loz", "<u4"), ("hix", "<u4"),
                    ("hiy", "<u4"), ("hiz", "<u4"), ("sy", "<f4"), ("sz", "<f4"), ("child", "<i4", (4,))])
TRI64_DT = np.dtype([("a", "<f4", (4,)), ("b", "<f4", (4,)), ("c", "<f4", (4,)), ("d", "<f4", (4,))])
TRI48_DT = np.dtype([("a", "<f4", (4,)), ("b", "<f4", (4,)), ("c", "<f4", (4,))])
FLOAT4_DT = np.dtype([("v", "<f4", (4,))])                      # a unit normal; node_box is [nodes][2] of these
COOP_DT = np.dtype([("lo_xy", "<u4"), ("loz_hix", "<u4"), ("hi_yz", "<u4"), ("ref", "<i4")])
assert (NODE_DT.itemsize, TRI64_DT.itemsize, TRI48_DT.itemsize, FLOAT4_DT.itemsize, COOP_DT.itemsize) == (64, 64, 48, 16, 16)

HEADER_FIELDS = ("nodes", "tris", "levels", "stack_need", "pad", "amax", "coop16_nodes", "coop_levels", "refit_pending", "fast")
MAX_BUILD_LEVELS = 96               # kMaxBuildLevels: d_coop_levels is [2][kMaxBuildLevels + 2]
NO_MATERIAL = 0xFFFF
EMPTY_COOP = (0x7C007C00, 0xFC007C00, 0xFC00FC00, 0)   # the inverted box (+inf, -inf), reference 0
WHAT = {"header": 0, "nodes": 1, "tri64": 2, "tri48": 3, "nrm": 4, "leaf_pos": 5, "level_begin": 6, "coop4": 7, "coop16": 8,
        "coop_levels": 9, "node_box": 10}
_DTYPES = {"nodes": NODE_DT, "tri64": TRI64_DT, "tri48": TRI48_DT, "nrm": FLOAT4_DT, "leaf_pos": np.dtype("<u4"),
           "level_begin": np.dtype("<i4"), "coop4": COOP_DT, "coop16": COOP_DT, "coop_levels": np.dtype("<i4"),
           "node_box": FLOAT4_DT}


class Tree:
    """One snapshot: header (dict) + the arrays named in WHAT"""

    def __init__(self, header, **arrays):
        self.header = dict(header)
        for k in _DTYPES:
            setattr(self, k, arrays.get(k))

    def copy(self):
        return Tree(self.header, **{k: (None if getattr(self, k) is None else getattr(self, k).copy()) for k in _DTYPES})


def fetch(ctx, name):
    """one array of the committed scene of a component.Context, through fs_debug_scene_snapshot ("header": a dict)"""
    fn = ctx.lib.fs_debug_scene_snapshot
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    what = WHAT[name]
    n = C.c_size_t(0)
    rc = fn(ctx.h, what, None, 0, C.byref(n))
    buf = np.zeros(n.value, np.uint8)
    if n.value == 0:
        ctx.check(rc)
    else:
        assert rc != 0, "a buffer of no bytes was accepted"       # too small: an error, with the size needed
        m = C.c_size_t(0)                                         # one byte short is still too small, and writes nothing
        assert fn(ctx.h, what, buf.ctypes.data, n.value - 1, C.byref(m)) != 0 and m.value == n.value and not buf.any()
        ctx.check(fn(ctx.h, what, buf.ctypes.data, n.value, C.byref(n)))
        assert n.value == buf.size
    if name == "header":
        assert buf.size == 48
        hdr = {k: int(v) for k, v in zip(HEADER_FIELDS, buf.view("<u4"))}
        hdr["pad"], hdr["amax"] = np.float32(buf.view("<f4")[4]), np.float32(buf.view("<f4")[5])
        return hdr
    a = buf.view(_DTYPES[name])
    return a.reshape(-1, 2) if name == "node_box" else a


def snapshot(ctx):
    """every array of the committed scene"""
    return Tree(fetch(ctx, "header"), **{k: fetch(ctx, k) for k in _DTYPES})


# ---- small soup generators (the kinds of tests/test_gpu_parity.py: test_line_trace_fuzz_soups) --------------------------------
SOUP_KINDS = ("uniform", "slivers", "duplicates", "zero_area", "tiny_and_big", "coplanar_grid")


def soup(kind, T, rng, offset=(0.0, 0.0, 0.0)):
    """T triangles [T][3][3] float32 of one kind (or "mixed": a part of every kind), shifted by `offset`"""
    T = int(T)
    if kind == "mixed":
        parts = [soup(k, n, rng) for k, n in zip(SOUP_KINDS, np.bincount(np.arange(T) % len(SOUP_KINDS), minlength=len(SOUP_KINDS))) if n]
        tri = np.concatenate(parts, axis=0).astype(np.float64)[rng.permutation(T)]
    elif kind == "uniform":
        tri = rng.uniform(-2000, 2000, (T, 1, 3)) + rng.normal(0, 60, (T, 3, 3))
    elif kind == "slivers":
        d = rng.normal(size=(T, 1, 3))
        t = np.array([0.0, 1.0, 0.5]).reshape(1, 3, 1)
        tri = rng.uniform(-1500, 1500, (T, 1, 3)) + d * t * rng.uniform(50, 900, (T, 1, 1)) + rng.normal(0, 0.02, (T, 3, 3))
    elif kind == "duplicates":
        n = max(1, (T + 2) // 3)
        base = rng.uniform(-800, 800, (n, 1, 3)) + rng.normal(0, 80, (n, 3, 3))
        tri = np.concatenate([base, base, base], axis=0)[:T]
    elif kind == "zero_area":
        tri = rng.uniform(-1500, 1500, (T, 1, 3)) + rng.normal(0, 70, (T, 3, 3))
        tri[0::4, 1] = tri[0::4, 0]                                             # two corners equal
        tri[1::4, 1] = tri[1::4, 0]; tri[1::4, 2] = tri[1::4, 0]                # all three equal
        tri[2::4, 2] = 0.5 * (tri[2::4, 0] + tri[2::4, 1])                      # three corners on a line
    elif kind == "tiny_and_big":
        tri = rng.uniform(-1000, 1000, (T, 1, 3)) + rng.normal(0, 1, (T, 3, 3)) * 10.0 ** rng.uniform(-1.5, 2.5, (T, 1, 1))
    elif kind == "coplanar_grid":
        n = int(np.ceil(np.sqrt((T + 1) // 2))) + 1
        xs, ys = np.meshgrid(np.arange(n) * 50.0, np.arange(n) * 50.0, indexing="ij")
        p = np.stack([xs, ys, np.zeros_like(xs)], -1)
        p00, p10, p01, p11 = p[:-1, :-1], p[1:, :-1], p[:-1, 1:], p[1:, 1:]
        tri = np.concatenate([np.stack([p00, p10, p11], -2).reshape(-1, 3, 3), np.stack([p00, p11, p01], -2).reshape(-1, 3, 3)])[:T]
    else:
        raise ValueError(kind)
    assert tri.shape == (T, 3, 3), (kind, tri.shape)
    return (tri + np.asarray(offset, np.float64)).astype(np.float32)


# ---- helpers --------------------------------------------------------------------------------------------------------
def _words(rec):
    """a record array as uint32 words [n][words]"""
    return np.ascontiguousarray(rec).view("<u4").reshape(rec.shape[0], rec.dtype.itemsize // 4)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view("<u4")


def _node_bytes(nodes):
    """lo, hi [n][child][axis] (int64), origin, step [n][axis] (float32)"""
    sh = 8 * np.arange(4, dtype=np.uint32)
    lo = np.stack([(nodes[k][:, None] >> sh) & 0xFF for k in ("lox", "loy", "loz")], axis=-1).astype(np.int64)
    hi = np.stack([(nodes[k][:, None] >> sh) & 0xFF for k in ("hix", "hiy", "hiz")], axis=-1).astype(np.int64)
    origin = np.stack([nodes["ox"], nodes["oy"], nodes["oz"]], axis=-1)
    step = np.stack([nodes["sx"], nodes["sy"], nodes["sz"]], axis=-1)
    return lo, hi, origin, step


def _used(nodes):
    """the refit's and the traversal's reading of a slot: used when lo <= hi on the x axis"""
    sh = 8 * np.arange(4, dtype=np.uint32)
    return ((nodes["lox"][:, None] >> sh) & 0xFF) <= ((nodes["hix"][:, None] >> sh) & 0xFF)


def _level_of(level_begin, n):
    lb = np.asarray(level_begin, np.int64)
    return np.searchsorted(lb, np.arange(n), side="right") - 1


def _levels_ok(tree):
    lb = np.asarray(tree.level_begin, np.int64)
    n = tree.nodes.shape[0]
    return lb.size >= 2 and lb[0] == 0 and lb[-1] == n and bool(np.all(np.diff(lb) > 0))


def refit_pad(header):
    """the padding fs_scene_refit and the builders use, in fp32: max(max(0.01f, amax * 3.8146973e-06f), bvh.pad)"""
    amax, pad = np.float32(header["amax"]), np.float32(header["pad"])
    return np.float32(max(max(np.float32(0.01), np.float32(amax * np.float32(3.8146973e-06))), pad))


def ulp32(x):
    """spacing of the float32 numbers at magnitude x"""
    return float(np.spacing(np.float32(abs(float(x)))))


def _fmt(idx, limit=4):
    idx = np.asarray(idx)
    return f"{idx.shape[0]} (first {idx[:limit].tolist()})"


# ---- a: topology ------------------------------------------------------------------------------------------------------
def check_topology(tree, device_build=False):
    """Levels tile the nodes; inner children lie one level down; every node but the root is referenced once; the used flag
    agrees on the three axes; leaf ranges cover [0, T) once; the input indices are a permutation that leaf_pos inverts; the
    pending-stack bound of a one-child-at-a-time descent (collapse_kernel's need[], bvh_check.cpp's max_pending) is at most
    the header's stack_need — and equal to it for a device build, whose kernel computes exactly this quantity."""
    f = []
    nodes, T, n = tree.nodes, tree.tri64.shape[0], tree.nodes.shape[0]
    hdr = tree.header
    if hdr["nodes"] != n or hdr["tris"] != T:
        f.append(f"topology.header: header says {hdr['nodes']} nodes / {hdr['tris']} triangles, arrays hold {n} / {T}")
    if T == 0:
        if n:
            f.append("topology.header: an empty scene has nodes")
        return f
    if not _levels_ok(tree):
        f.append(f"topology.levels: level ranges {np.asarray(tree.level_begin).tolist()[:12]} do not tile [0, {n}) without an empty level")
        return f
    lb = np.asarray(tree.level_begin, np.int64)
    levels = lb.size - 1
    if hdr["levels"] != levels:
        f.append(f"topology.levels: header says {hdr['levels']} levels, level_begin has {levels}")
    lo, hi, _, _ = _node_bytes(nodes)
    used3 = lo <= hi                                   # [n][c][axis]
    used = used3[..., 0]
    bad = np.argwhere(used3.any(-1) != used3.all(-1))
    if bad.size:
        f.append(f"topology.used_flag: the axes disagree on whether a slot is used at (node, child) {_fmt(bad)}")
    empty = ~used3.any(-1)
    bad = np.argwhere(empty & ~((lo == 255).all(-1) & (hi == 0).all(-1)))
    if bad.size:
        f.append(f"topology.empty_slot: an empty slot does not hold lo = 255 / hi = 0 on every axis at (node, child) {_fmt(bad)}")
    child = nodes["child"].astype(np.int64)
    lvl = _level_of(lb, n)
    inner = used & (child >= 0)
    leaf = used & (child < 0)
    pn, pc = np.nonzero(inner)
    tgt = child[pn, pc]
    in_range = tgt < n
    if not in_range.all():
        f.append(f"topology.child_range: inner links beyond the node array at (node, child) {_fmt(np.stack([pn, pc], 1)[~in_range])}")
    wrong = in_range.copy()
    wrong[in_range] = lvl[tgt[in_range]] != lvl[pn[in_range]] + 1
    if wrong.any():
        f.append(f"topology.child_level: inner children not exactly one level below their parent at (node, child) {_fmt(np.stack([pn, pc], 1)[wrong])}")
    refs = np.bincount(tgt[in_range], minlength=n)
    expect = np.ones(n, np.int64); expect[0] = 0
    bad = np.nonzero(refs != expect)[0]
    if bad.size:
        f.append(f"topology.references: nodes not referenced exactly once (the root: never) {_fmt(bad)}")
    # leaves
    code = ~child[leaf]
    first, cnt = code >> 2, (code & 3) + 1
    most = 2 if device_build else 4
    if (cnt > most).any():
        f.append(f"topology.leaf_count: leaves of more than {most} triangles: {int((cnt > most).sum())}")
    if (first + cnt > T).any():
        f.append(f"topology.leaf_cover: leaf ranges beyond [0, {T}): {int((first + cnt > T).sum())}")
    else:
        cover = np.zeros(T + 1, np.int64)
        np.add.at(cover, first, 1)
        np.add.at(cover, first + cnt, -1)
        cover = np.cumsum(cover)[:T]
        bad = np.nonzero(cover != 1)[0]
        if bad.size:
            f.append(f"topology.leaf_cover: leaf-order positions not covered exactly once {_fmt(bad)} (x{cover[bad[:4]].tolist()})")
    # the permutation
    idx = _words(tree.tri64)[:, 10].astype(np.int64)
    if not np.array_equal(np.sort(idx), np.arange(T)):
        f.append("topology.permutation: the input indices in Tri64.c.z are not a permutation of [0, T)")
    elif tree.leaf_pos.shape[0] != T or not np.array_equal(tree.leaf_pos.astype(np.int64)[idx], np.arange(T)):
        bad = np.nonzero(tree.leaf_pos.astype(np.int64)[idx] != np.arange(T))[0] if tree.leaf_pos.shape[0] == T else np.arange(0)
        f.append(f"topology.leaf_pos: leaf_pos does not invert the leaf order at positions {_fmt(bad)}")
    # the stack bound, level by level: need[child] = need[parent] + children(parent) - 1
    if not any(s.startswith(("topology.child_range", "topology.child_level", "topology.references")) for s in f):
        need = np.zeros(n, np.int64)
        nchild = used.sum(1)
        worst = 0
        for l in range(levels):
            a, b = lb[l], lb[l + 1]
            here = need[a:b] + nchild[a:b] - 1
            worst = max(worst, int(here.max()))
            m = inner[a:b]
            need[child[a:b][m]] = np.broadcast_to(here[:, None], m.shape)[m]
        if worst > hdr["stack_need"]:
            f.append(f"topology.stack_need: the tree needs {worst} pending entries, the header says {hdr['stack_need']}")
        elif device_build and worst != hdr["stack_need"]:
            f.append(f"topology.stack_need: the device build reports {hdr['stack_need']}, the tree needs {worst}")
    return f


# ---- b: records -------------------------------------------------------------------------------------------------------
def check_records(tree, tri_in, mat=None, obj=None, host_tri64=None):
    """Tri48 and the normals are the matching words of Tri64; v0, e1, e2 are the inputs and their fp32 differences by bits;
    material and object words are the inputs'; with `host_tri64` (the records of a host commit of the same triangles in
    another context) every whole record equals the host's bit for bit, matched by input index — NaN normals of triangles
    without area included, as bit patterns.  tri_in [T][3][3] float32 = the positions the scene holds now."""
    f = []
    T = tree.tri64.shape[0]
    w = _words(tree.tri64)
    bad = np.nonzero((_words(tree.tri48) != w[:, :12]).any(1))[0] if tree.tri48.shape[0] == T else np.arange(T)
    if bad.size:
        f.append(f"records.tri48: Tri48 differs from the first 48 bytes of Tri64 at positions {_fmt(bad)}")
    bad = np.nonzero((_words(tree.nrm) != w[:, 12:]).any(1))[0] if tree.nrm.shape[0] == T else np.arange(T)
    if bad.size:
        f.append(f"records.normal: the normal array differs from Tri64.d at positions {_fmt(bad)}")
    if T == 0:
        return f
    idx = w[:, 10].astype(np.int64)
    if idx.max() >= T or tri_in.shape[0] != T:
        f.append("records.index: input index out of range")
        return f
    p = np.ascontiguousarray(tri_in, np.float32)[idx]
    want = np.concatenate([p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], axis=1)   # fp32 differences
    bad = np.nonzero((_bits(want) != w[:, :9]).any(1))[0]
    if bad.size:
        f.append(f"records.vertices: v0 / e1 / e2 differ from the inputs and their fp32 differences at positions {_fmt(bad)}")
    m = np.full(T, NO_MATERIAL, np.uint32) if mat is None else np.asarray(mat).astype(np.uint32)
    o = np.arange(T, dtype=np.uint32) if obj is None else np.asarray(obj).astype(np.uint32)
    if (w[:, 9] != m[idx]).any():
        f.append(f"records.material: material words differ from the inputs at positions {_fmt(np.nonzero(w[:, 9] != m[idx])[0])}")
    if (w[:, 11] != o[idx]).any():
        f.append(f"records.object: object words differ from the inputs at positions {_fmt(np.nonzero(w[:, 11] != o[idx])[0])}")
    if host_tri64 is not None:
        hw = _words(host_tri64)
        if hw.shape != w.shape or not np.array_equal(np.sort(hw[:, 10]), np.arange(T)):
            f.append("records.host: the host commit's records are not a permutation of the same triangles")
        else:
            diff = w[np.argsort(idx)] != hw[np.argsort(hw[:, 10])]
            if diff.any():
                t = np.nonzero(diff.any(1))[0]
                f.append(f"records.host: records differ from the host commit's at input triangles {_fmt(t)}, words {np.nonzero(diff.any(0))[0].tolist()}"
                         f" (first: {w[np.argsort(idx)][t[0]][diff[t[0]]].tolist()} against {hw[np.argsort(hw[:, 10])][t[0]][diff[t[0]]].tolist()})")
    return f


# ---- bounds below every child ----------------------------------------------------------------------------------------------
def _tri_bounds(tree, dtype, tri_in=None):
    """per leaf-order position: lo, hi [T][3].  From the input vertices when given (what the host builder boxes), else from
    the records as refit_level_kernel reads them: v0, v0 + e1, v0 + e2 in `dtype` (float32: the kernel's own sums)."""
    t = tree.tri64
    if tri_in is not None:
        idx = _words(t)[:, 10].astype(np.int64)
        v = np.ascontiguousarray(tri_in, np.float32)[idx].astype(dtype)
    else:
        v0 = t["a"][:, :3].astype(dtype)
        e1 = np.stack([t["a"][:, 3], t["b"][:, 0], t["b"][:, 1]], 1).astype(dtype)
        e2 = np.stack([t["b"][:, 2], t["b"][:, 3], t["c"][:, 0]], 1).astype(dtype)
        v = np.stack([v0, v0 + e1, v0 + e2], axis=1)
    return v.min(1), v.max(1)


def derive_boxes(tree, dtype=np.float32, tri_in=None):
    """child boxes [n][4][3] and node boxes [n][3] (lo, hi each), bottom-up, one pass per level; min / max are exact in any
    format, so with float32 this is bit for bit what refit_level_kernel derives.  Unused slots: (+inf, -inf)."""
    nodes, n, T = tree.nodes, tree.nodes.shape[0], tree.tri64.shape[0]
    lb = np.asarray(tree.level_begin, np.int64)
    tlo, thi = _tri_bounds(tree, dtype, tri_in)
    tlo = np.concatenate([tlo, np.full((4, 3), np.inf, dtype)])      # (a leaf range is read up to 3 places past its end)
    thi = np.concatenate([thi, np.full((4, 3), -np.inf, dtype)])
    used = _used(nodes)
    child = nodes["child"].astype(np.int64)
    cb_lo = np.full((n, 4, 3), np.inf, dtype); cb_hi = np.full((n, 4, 3), -np.inf, dtype)
    nb_lo = np.full((n, 3), np.inf, dtype); nb_hi = np.full((n, 3), -np.inf, dtype)
    for l in range(lb.size - 2, -1, -1):
        a, b = lb[l], lb[l + 1]
        u, ch = used[a:b], child[a:b]
        lo = np.full((b - a, 4, 3), np.inf, dtype); hi = np.full((b - a, 4, 3), -np.inf, dtype)
        inner = u & (ch >= 0)
        lo[inner] = nb_lo[ch[inner]]; hi[inner] = nb_hi[ch[inner]]
        leaf = u & (ch < 0)
        code = ~ch[leaf]
        first, cnt = np.clip(code >> 2, 0, T), (code & 3) + 1
        llo = np.full((first.shape[0], 3), np.inf, dtype); lhi = np.full((first.shape[0], 3), -np.inf, dtype)
        for j in range(4):
            m = (cnt > j)[:, None]
            llo = np.where(m, np.minimum(llo, tlo[first + j]), llo)
            lhi = np.where(m, np.maximum(lhi, thi[first + j]), lhi)
        lo[leaf] = llo; hi[leaf] = lhi
        cb_lo[a:b] = lo; cb_hi[a:b] = hi
        nb_lo[a:b] = lo.min(1); nb_hi[a:b] = hi.max(1)
    return cb_lo, cb_hi, nb_lo, nb_hi


def _min_step(ext):
    """the smallest power of two s with 255 s >= ext (float64, exact: 255 * 2^e is a float64)"""
    m, e = np.frexp(ext / 255.0)
    e = np.where(m == 0.5, e - 1, e).astype(np.int64)
    e = np.where(np.ldexp(255.0, e) < ext, e + 1, e)           # the division may have rounded either way
    e = np.where(np.ldexp(255.0, e - 1) >= ext, e - 1, e)
    return np.ldexp(1.0, np.clip(e, -100, 100))


# ---- c: box invariants -----------------------------------------------------------------------------------------------------
def check_boxes(tree, tri_in=None, amax_expected=None):
    """For any committed tree.  With pad = refit_pad(header), box = origin + q * step decoded in float64, and the tight
    bounds t of everything below a child (the fp32 sums v0 + e1, v0 + e2 of the records, or the input vertices if `tri_in`
    is given: a host-built tree as uploaded boxes those):
      * every step is a power of two, 255 * step covers the node's padded extent, and the half step would not (a step
        twice the minimum passes only where the builders' log2 may round across an integer: within 2^-40 of one).  The
        builders round each padded side to fp32, half an ulp32(amax + pad) each, so the extent is known here to one such
        ulp: that much is allowed either way (check d, which has the kernel's own extent, allows nothing);
      * a used child box contains t with at least pad / 2 to spare on each side (bvh_check.cpp's margin; it covers the
        1.5 ulp32(amax) between v0 + e1 and the input vertex and the half ulp of the float origin: pad >= amax * 2^-18);
      * no side stands off from t by more than pad + step + ulp32(amax).  Derivation for the low side (the high side
        mirrors it): the plane is o + floor(l) * step with l = (fl32(t - pad) - o) / step >= 0, so it lies less than one
        step below fl32(t - pad) — the clamp to 0 only raises it, to o <= fl32(t - pad) — and fl32(t - pad) lies at most
        half an ulp32(|t| + pad) <= ulp32(amax) below t - pad.  Nothing here is measured.
      * amax equals the largest |coordinate| the test supplied (`amax_expected`)."""
    f = []
    hdr = tree.header
    n, T = tree.nodes.shape[0], tree.tri64.shape[0]
    if amax_expected is not None and np.float32(hdr["amax"]) != np.float32(amax_expected):
        f.append(f"box.amax: header says {hdr['amax']!r}, the coordinates supplied reach {np.float32(amax_expected)!r}")
    if T == 0 or n == 0 or not _levels_ok(tree):
        return f
    pad = float(refit_pad(hdr))
    amax = float(hdr["amax"])
    lo, hi, origin, step = _node_bytes(tree.nodes)
    m, _ = np.frexp(step.astype(np.float64))
    bad = np.argwhere(~((step > 0) & (m == 0.5)))
    if bad.size:
        f.append(f"box.step_pow2: grid steps that are no power of two at (node, axis) {_fmt(bad)}")
        return f
    cb_lo, cb_hi, nb_lo, nb_hi = derive_boxes(tree, np.float32, tri_in)
    cb_lo, cb_hi, nb_lo, nb_hi = (x.astype(np.float64) for x in (cb_lo, cb_hi, nb_lo, nb_hi))
    step64, o64 = step.astype(np.float64), origin.astype(np.float64)
    u = ulp32(amax + pad)
    ext = (nb_hi - nb_lo) + 2.0 * pad                            # the builders round each padded side to fp32: +- u in all
    bad = np.argwhere(255.0 * step64 < ext - u)
    if bad.size:
        f.append(f"box.step_small: 255 steps do not cover the node's padded extent at (node, axis) {_fmt(bad)}")
    bad = np.argwhere(255.0 * (step64 / 2) >= (ext + u) * (1.0 + 2.0 ** -40))
    if bad.size:
        f.append(f"box.step_loose: half the grid step would cover the node's padded extent at (node, axis) {_fmt(bad)}")
    used = _used(tree.nodes)
    dlo = o64[:, None, :] + lo * step64[:, None, :]
    dhi = o64[:, None, :] + hi * step64[:, None, :]
    room_lo, room_hi = cb_lo - dlo, dhi - cb_hi                  # >= pad / 2 wanted, <= pad + step + ulp wanted
    um = used[..., None] & np.ones(3, bool)
    bad = np.argwhere(um & ~((room_lo >= pad / 2) & (room_hi >= pad / 2)))
    if bad.size:
        i, c, k = bad[0]
        f.append(f"box.margin: child boxes with less than pad / 2 = {pad / 2:g} around what lies below them at (node, child, axis) {_fmt(bad)}:"
                 f" [{float(dlo[i, c, k])!r}, {float(dhi[i, c, k])!r}] around [{float(cb_lo[i, c, k])!r}, {float(cb_hi[i, c, k])!r}]")
    limit = pad + step64[:, None, :] + ulp32(amax)
    bad = np.argwhere(um & ~((room_lo <= limit) & (room_hi <= limit)))
    if bad.size:
        i, c, k = bad[0]
        f.append(f"box.loose: child boxes standing off by more than pad + step + ulp at (node, child, axis) {_fmt(bad)}:"
                 f" [{float(dlo[i, c, k])!r}, {float(dhi[i, c, k])!r}] around [{float(cb_lo[i, c, k])!r}, {float(cb_hi[i, c, k])!r}], step {float(step64[i, k])!r}")
    return f


# ---- d: refit_level_kernel ---------------------------------------------------------------------------------------------------
def restate_refit(tree, pad, own_step=False):
    """refit_level_kernel on the tree's topology and Tri64: (nodes, node_box).  own_step: keep every node's stored grid step
    (the bytes are then exact whatever log2 did); else the minimal one.  Slots keep their used / empty state."""
    pad = np.float32(pad)
    nodes = tree.nodes.copy()
    n = nodes.shape[0]
    cb_lo, cb_hi, nb_lo, nb_hi = derive_boxes(tree, np.float32)
    node_box = np.zeros((n, 2), FLOAT4_DT)
    node_box["v"][:, 0, :3] = nb_lo; node_box["v"][:, 1, :3] = nb_hi
    with np.errstate(invalid="ignore", over="ignore"):
        originf = (nb_lo - pad).astype(np.float32)
        ext = (nb_hi + pad).astype(np.float32).astype(np.float64) - originf.astype(np.float64)
        step = np.stack([nodes["sx"], nodes["sy"], nodes["sz"]], 1).astype(np.float64) if own_step else _min_step(np.maximum(ext, 1e-30))
        l = ((cb_lo - pad).astype(np.float32).astype(np.float64) - originf.astype(np.float64)[:, None, :]) / step[:, None, :]
        h = ((cb_hi + pad).astype(np.float32).astype(np.float64) - originf.astype(np.float64)[:, None, :]) / step[:, None, :]
        used = _used(tree.nodes)[..., None] & np.ones(3, bool)
        ql = np.where(used, np.clip(np.floor(np.where(used, l, 0.0)), 0, 255), 255).astype(np.uint32)
        qh = np.where(used, np.clip(np.ceil(np.where(used, h, 0.0)), 0, 255), 0).astype(np.uint32)
    sh = 8 * np.arange(4, dtype=np.uint32)[None, :, None]
    lo4 = (ql << sh).sum(1).astype(np.uint32); hi4 = (qh << sh).sum(1).astype(np.uint32)
    for k, ax in enumerate("xyz"):
        nodes["o" + ax] = originf[:, k]
        nodes["s" + ax] = step[:, k].astype(np.float32)
        nodes["lo" + ax] = lo4[:, k]; nodes["hi" + ax] = hi4[:, k]
    return nodes, node_box, ext


def check_refit(tree, pad=None):
    """refit_level_kernel restated exactly (device builds, any tree after fs_scene_refit): child and node boxes from Tri64
    with fp32 min / max and the fp32 sums v0 + e1, v0 + e2; node_box and the origins by bits (min / max of +0 and -0 may
    return either: zeros are compared by value); the step is the minimal power of two — or twice it where the padded
    extent lies within 2^-40 of 255 times a power of two, since log2 may round across the integer there; with the node's
    own step the lo / hi bytes are recomputed in float64 exactly as the kernel does and must be equal."""
    f = []
    if tree.nodes.shape[0] == 0 or not _levels_ok(tree):
        return f
    pad = refit_pad(tree.header) if pad is None else np.float32(pad)
    want, box, ext = restate_refit(tree, pad, own_step=True)
    have = tree.nodes
    if tree.node_box is None or tree.node_box.shape != box.shape:
        f.append("refit.node_box: no node_box array of the tree's size")
    else:
        a, b = tree.node_box["v"] + np.float32(0), box["v"] + np.float32(0)      # -0 -> +0
        bad = np.nonzero((_bits(a) != _bits(b)).reshape(a.shape[0], -1).any(1))[0]
        if bad.size:
            f.append(f"refit.node_box: node_box differs from the fp32 bounds of the records at nodes {_fmt(bad)}")
    for ax in "xyz":
        bad = np.nonzero(_bits(have["o" + ax]) != _bits(want["o" + ax]))[0]
        if bad.size:
            f.append(f"refit.origin: origin.{ax} differs from fl32(lo - pad) at nodes {_fmt(bad)}: {have['o' + ax][bad[0]]!r} against {want['o' + ax][bad[0]]!r}")
    step = np.stack([have["sx"], have["sy"], have["sz"]], 1).astype(np.float64)
    smin = _min_step(np.maximum(ext, 1e-30))
    edge = ext >= 255.0 * smin * (1.0 - 2.0 ** -40)
    bad = np.argwhere(~((step == smin) | ((step == 2 * smin) & edge)))
    if bad.size:
        i, k = bad[0]
        f.append(f"refit.step: grid steps that are not the smallest power of two covering the padded extent at (node, axis) {_fmt(bad)}:"
                 f" {float(step[i, k])!r} for an extent of {float(ext[i, k])!r}")
    for k in ("lox", "loy", "loz", "hix", "hiy", "hiz"):
        bad = np.nonzero(have[k] != want[k])[0]
        if bad.size:
            f.append(f"refit.bytes: {k} differs from the exact outward rounding at nodes {_fmt(bad)}: {int(have[k][bad[0]]):#010x} against {int(want[k][bad[0]]):#010x}")
    return f


# ---- e: coop_nodes_kernel ----------------------------------------------------------------------------------------------------
def _h_dec(b):   # toward -inf, on fp16 bit patterns
    b = b.astype(np.uint16)
    return np.where((b & 0x7FFF) == 0, np.uint16(0x8001), np.where((b & 0x8000) != 0, b + np.uint16(1), b - np.uint16(1))).astype(np.uint16)


def _h_inc(b):   # toward +inf
    b = b.astype(np.uint16)
    return np.where((b & 0x7FFF) == 0, np.uint16(0x0001), np.where((b & 0x8000) != 0, b - np.uint16(1), b + np.uint16(1))).astype(np.uint16)


def _h_val(b):
    return b.astype(np.uint16).view(np.float16).astype(np.float32)


def h_below(x):
    """fs_refit.hip: an fp16 strictly below the finite float32 x, as a bit pattern (0xFC00 = -inf stays)"""
    with np.errstate(over="ignore"):
        b = x.astype(np.float32).astype(np.float16).view(np.uint16)      # round to nearest even, overflow to infinity
    minf = b == 0xFC00
    b = np.where(~minf & (_h_val(b) > x), _h_dec(b), b)
    return np.where(minf | (b == 0xFC00), b, _h_dec(b)).astype(np.uint16)


def h_above(x):
    with np.errstate(over="ignore"):
        b = x.astype(np.float32).astype(np.float16).view(np.uint16)
    pinf = b == 0x7C00
    b = np.where(~pinf & (_h_val(b) < x), _h_inc(b), b)
    return np.where(pinf | (b == 0x7C00), b, _h_inc(b)).astype(np.uint16)


def restate_coop4(nodes):
    """coop_nodes_kernel: CoopChild[4 n].  The plane fmaf(q, step, origin) is float32(q * step + origin) with the sum exact
    in float64: q has 8 bits, step is a power of two >= 2^-25 amax and |origin| <= 2 amax, so the sum spans < 53 bits."""
    lo, hi, origin, step = _node_bytes(nodes)
    o, s = origin.astype(np.float64)[:, None, :], step.astype(np.float64)[:, None, :]
    with np.errstate(over="ignore"):
        plo = (lo * s + o).astype(np.float32); phi = (hi * s + o).astype(np.float32)
    used = (lo <= hi).all(-1)
    um = used[..., None] & np.ones(3, bool)
    blo = np.where(um, h_below(plo), np.uint16(0x7C00)).astype(np.uint32)
    bhi = np.where(um, h_above(phi), np.uint16(0xFC00)).astype(np.uint32)
    out = np.zeros((nodes.shape[0], 4), COOP_DT)
    out["lo_xy"] = blo[..., 0] | (blo[..., 1] << 16)
    out["loz_hix"] = blo[..., 2] | (bhi[..., 0] << 16)
    out["hi_yz"] = bhi[..., 1] | (bhi[..., 2] << 16)
    out["ref"] = np.where(used, nodes["child"], 0)
    return out.reshape(-1)


def _compare_coop(code, have, want, what):
    f = []
    if have is None or have.shape != want.shape:
        return [f"{code}.size: {what} holds {None if have is None else have.shape[0]} records, {want.shape[0]} expected"]
    box = (have["lo_xy"] != want["lo_xy"]) | (have["loz_hix"] != want["loz_hix"]) | (have["hi_yz"] != want["hi_yz"])
    if box.any():
        i = np.nonzero(box)[0]
        f.append(f"{code}.box: fp16 planes of {what} differ at records {_fmt(i)}: "
                 f"{[hex(int(have[k][i[0]])) for k in ('lo_xy', 'loz_hix', 'hi_yz')]} against {[hex(int(want[k][i[0]])) for k in ('lo_xy', 'loz_hix', 'hi_yz')]}")
    ref = have["ref"] != want["ref"]
    if ref.any():
        i = np.nonzero(ref)[0]
        f.append(f"{code}.ref: references of {what} differ at records {_fmt(i)}: {int(have['ref'][i[0]])} against {int(want['ref'][i[0]])}")
    return f


def check_coop4(tree):
    """all 4 * nodes records of the cooperative traversal's per-child array against restate_coop4, by bits"""
    if tree.nodes.shape[0] == 0:
        return []
    return _compare_coop("coop4", tree.coop4, restate_coop4(tree.nodes), "the per-child array")


def has_infinite_planes(coop):
    h = np.stack([coop["lo_xy"] & 0xFFFF, coop["lo_xy"] >> 16, coop["loz_hix"] & 0xFFFF, coop["loz_hix"] >> 16,
                  coop["hi_yz"] & 0xFFFF, coop["hi_yz"] >> 16], 1)
    empty = (coop["lo_xy"] == EMPTY_COOP[0]) & (coop["loz_hix"] == EMPTY_COOP[1])
    return bool((((h & 0x7FFF) == 0x7C00).any(1) & ~empty).any())


# ---- f: coop16_kernel ----------------------------------------------------------------------------------------------------------
def dense_table(level_begin):
    """refresh_coop_nodes: (table [2][kMaxBuildLevels + 2] = level_begin | first dense index of every even level, coop16_nodes)"""
    lb = np.asarray(level_begin, np.int64)
    levels = lb.size - 1
    tab = np.full((2, MAX_BUILD_LEVELS + 2), -1, np.int32)
    tab[0, :levels + 1] = lb
    n16 = 0
    for l in range(0, levels, 2):
        tab[1, l] = n16
        n16 += int(lb[l + 1] - lb[l])
    return tab, n16


def restate_coop16(coop4, level_begin):
    """coop16_kernel: for node X of an even level and its child c — a leaf: its record in slot 4c; an inner node Y: the
    records of Y's four children in slots 4c .. 4c + 3, their inner references renumbered into the even levels' dense order"""
    lb = np.asarray(level_begin, np.int64)
    tab, n16 = dense_table(lb)
    levels = lb.size - 1
    X = np.concatenate([np.arange(lb[l], lb[l + 1]) for l in range(0, levels, 2)]) if levels > 0 else np.arange(0)
    lvl = _level_of(lb, int(lb[-1]))[X]
    c4 = coop4.reshape(-1, 4)
    out = np.zeros((n16, 4, 4), COOP_DT)
    for k, v in zip(COOP_DT.names, EMPTY_COOP):
        out[k] = v
    xc = c4[X]                                                           # [n16][c]
    x_empty = (xc["lo_xy"] == EMPTY_COOP[0]) & (xc["loz_hix"] == EMPTY_COOP[1])
    leaf = ~x_empty & (xc["ref"] < 0)
    g0 = out[:, :, 0]
    g0[leaf] = xc[leaf]
    out[:, :, 0] = g0
    inner = ~x_empty & (xc["ref"] >= 0)
    yi = np.clip(xc["ref"], 0, c4.shape[0] - 1)
    yc = c4[yi]                                                          # [n16][c][g]
    y_empty = (yc["lo_xy"] == EMPTY_COOP[0]) & (yc["loz_hix"] == EMPTY_COOP[1])
    nxt = np.minimum(lvl + 2, MAX_BUILD_LEVELS + 1)
    renum = tab[1][nxt][:, None, None] + (yc["ref"].astype(np.int64) - tab[0][nxt][:, None, None])
    yc = yc.copy()
    yc["ref"] = np.where(yc["ref"] >= 0, renum, yc["ref"]).astype(np.int32)
    take = inner[..., None] & ~y_empty
    out[take] = yc[take]
    return out.reshape(-1), tab, n16


def check_coop16(tree):
    """the dense table and coop16_nodes from level_begin as refresh_coop_nodes computes them, then all 16 * coop16_nodes
    records against restate_coop16 applied to the snapshot's own per-child array, by bits"""
    f = []
    if tree.nodes.shape[0] == 0 or not _levels_ok(tree):
        return f
    if tree.coop4 is None or tree.coop4.shape[0] != 4 * tree.nodes.shape[0]:
        return ["coop16.size: no per-child array to fold"]
    want, tab, n16 = restate_coop16(tree.coop4, tree.level_begin)
    levels = np.asarray(tree.level_begin).size - 1
    if tree.header["coop16_nodes"] != n16 or tree.header["coop_levels"] != levels:
        f.append(f"coop16.header: header says {tree.header['coop16_nodes']} 16-wide nodes in {tree.header['coop_levels']} levels, the level table gives {n16} in {levels}")
    if tree.coop_levels is None or not np.array_equal(np.asarray(tree.coop_levels).reshape(-1), tab.reshape(-1)):
        f.append("coop16.table: the device's level / dense table differs from the one level_begin gives")
    return f + _compare_coop("coop16", tree.coop16, want, "the 16-wide array")


def check_all(tree, tri_in, mat=None, obj=None, host_tri64=None, device_build=False, refitted=False, amax_expected=None):
    """checks a to f as they apply: d for device builds and refitted trees only (a host-built tree as uploaded holds the
    boxes of the input vertices, not of v0 + e1)"""
    derived = device_build or refitted
    f = check_topology(tree, device_build=device_build)
    f += check_records(tree, tri_in, mat, obj, host_tri64)
    if any(s.startswith("topology.") and not s.startswith("topology.stack_need") for s in f):
        return f                                     # the other restatements walk the tree: they need a sound one
    f += check_boxes(tree, None if derived else tri_in, amax_expected)
    if derived:
        f += check_refit(tree)
    f += check_coop4(tree)
    f += check_coop16(tree)
    return f
