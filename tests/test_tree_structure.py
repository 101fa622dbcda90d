"""Every device-written tree array against an exact restatement (tests/tree_check.py), not only along sampled rays.

CPU part: a small valid tree built in numpy passes the checker, and each of a list of faults the rays of the other tests
cannot see is reported with its own finding — which is what proves that the GPU part can fail.  GPU part: the committed
scene is read back through fs_debug_scene_snapshot and checks a to f run on it as they apply, over the sizes at which the
build kernels change path, large coordinates, moving geometry, re-registration and the progressive commit.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_check as tc  # noqa: E402


# ---- CPU: the checker on a synthetic tree ------------------------------------------------------------------------------------
def synth_tree(seed, levels):
    """a random 4-wide topology of `levels` levels, breadth-first, leaves of 1 and 2 triangles, filled through the
    restatements d to f; returns (tree, input triangles, materials)"""
    rng = np.random.default_rng(seed)
    level_begin, children, tcount = [0], [], 0          # children[node] = list of ("inner", index) / ("leaf", first, count)
    this_level = [0]
    next_index = 1
    for l in range(levels):
        nxt = []
        for j, node in enumerate(this_level):
            ch = []
            for c in range(int(rng.integers(2, 5))):
                if l < levels - 1 and ((j == 0 and c == 1) or rng.random() < 0.45):
                    ch.append(("inner", next_index)); nxt.append(next_index); next_index += 1
                else:
                    cnt = int(rng.integers(1, 3))
                    ch.append(("leaf", tcount, cnt)); tcount += cnt
            children.append(ch)
        level_begin.append(level_begin[-1] + len(this_level))
        this_level = nxt
    n, T = len(children), tcount
    tri_in = (rng.uniform(-2000, 2000, (T, 1, 3)) + rng.normal(0, 60, (T, 3, 3))).astype(np.float32)
    tri_in[T - 1, 2] = tri_in[T - 1, 0]                                     # one triangle without area
    mat = rng.integers(0, 3, T).astype(np.uint16)
    order = rng.permutation(T)                                              # leaf-order position -> input triangle
    p = tri_in[order]
    tri64 = np.zeros(T, tc.TRI64_DT)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.cross(e1.astype(np.float64), e2.astype(np.float64))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    w = tri64.view("<u4").reshape(T, 16)
    w[:, 0:3] = p[:, 0].view("<u4"); w[:, 3:6] = e1.view("<u4"); w[:, 6:9] = e2.view("<u4")
    w[:, 9] = mat[order]; w[:, 10] = order; w[:, 11] = order
    w[:, 12:15] = nrm.view("<u4")
    leaf_pos = np.zeros(T, np.uint32); leaf_pos[order] = np.arange(T)
    nodes = np.zeros(n, tc.NODE_DT)
    for i, ch in enumerate(children):
        lo4 = hi4 = 0
        for c in range(4):
            if c < len(ch):
                nodes["child"][i, c] = ch[c][1] if ch[c][0] == "inner" else ~(ch[c][1] * 4 + ch[c][2] - 1)
                hi4 |= 255 << (8 * c)
            else:
                nodes["child"][i, c] = -1
                lo4 |= 255 << (8 * c)
        for k in ("lox", "loy", "loz"):
            nodes[k][i] = lo4
        for k in ("hix", "hiy", "hiz"):
            nodes[k][i] = hi4

    def need(i, pending):                                                   # the stack bound, by plain recursion
        here = pending + len(children[i]) - 1
        return max([here] + [need(c[1], here) for c in children[i] if c[0] == "inner"])
    amax = np.float32(np.abs(tri_in).max())
    hdr = dict(nodes=n, tris=T, levels=levels, stack_need=need(0, 0), pad=np.float32(max(np.float32(0.01), amax * np.float32(3.8146973e-06))),
               amax=amax, coop16_nodes=0, coop_levels=levels, refit_pending=0, fast=1)
    tree = tc.Tree(hdr, nodes=nodes, tri64=tri64, tri48=tri64.view("<u4").reshape(T, 16)[:, :12].copy().view(tc.TRI48_DT).reshape(T),
                   nrm=tri64["d"].copy().view(tc.FLOAT4_DT).reshape(T), leaf_pos=leaf_pos, level_begin=np.array(level_begin, np.int32))
    refill(tree)
    return tree, tri_in, mat


def refill(tree, coop16=True):
    """boxes and cooperative arrays from the records, through restatements d to f"""
    tree.nodes, tree.node_box, _ = tc.restate_refit(tree, tc.refit_pad(tree.header))
    tree.coop4 = tc.restate_coop4(tree.nodes)
    if coop16:
        tree.coop16, tab, n16 = tc.restate_coop16(tree.coop4, tree.level_begin)
        tree.coop_levels = tab.reshape(-1)
        tree.header["coop16_nodes"] = n16


def run_checks(tree, tri_in, mat):
    return tc.check_all(tree, tri_in, mat, device_build=True, amax_expected=np.abs(tri_in).max())


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_checker_accepts_a_valid_tree(levels):
    for seed in range(4):
        tree, tri_in, mat = synth_tree(100 * levels + seed, levels)
        assert tree.level_begin.size == levels + 1 and np.all(np.diff(tree.level_begin) > 0)
        assert run_checks(tree, tri_in, mat) == []
        assert tc.check_all(tree, tri_in, mat, device_build=False, refitted=True) == []


def _set_byte(word, c, v):
    return (int(word) & ~(0xFF << (8 * c))) | (int(v) << (8 * c))


def _pick_plane(tree, side):
    """a used (node, child, axis) with a coarse grid (step >= 1 >> pad) whose `side` byte leaves room to move"""
    lo, hi, _, step = tc._node_bytes(tree.nodes)
    ok = tc._used(tree.nodes)[..., None] & (step[:, None, :] >= 1.0) & ((lo >= 2) if side == "lo" else (hi >= 1))
    assert ok.any()
    return tuple(int(v) for v in np.argwhere(ok)[0])


def m_hi_byte_lowered(tree, tri_in):
    # the plane of this child is set by a vertex: one step (>= 1, a hundred times the padding) further in, the vertex is outside
    i, c, k = _pick_plane(tree, "hi")
    name = "hi" + "xyz"[k]
    hi = (int(tree.nodes[name][i]) >> (8 * c)) & 0xFF
    tree.nodes[name][i] = _set_byte(tree.nodes[name][i], c, hi - 1)
    return ["box.margin", "refit.bytes"]


def m_lo_byte_lowered_by_two(tree, tri_in):
    i, c, k = _pick_plane(tree, "lo")
    name = "lo" + "xyz"[k]
    lo = (int(tree.nodes[name][i]) >> (8 * c)) & 0xFF
    tree.nodes[name][i] = _set_byte(tree.nodes[name][i], c, lo - 2)
    return ["box.loose", "refit.bytes"]


def m_leaf_ranges_overlap(tree, tri_in):
    ch = tree.nodes["child"]
    i, c = [tuple(x) for x in np.argwhere(tc._used(tree.nodes) & (ch < 0) & ((~ch >> 2) > 0))][0]
    ch[i, c] = ~(~int(ch[i, c]) - 4)                                     # the range starts one triangle early
    return ["topology.leaf_cover"]


def m_child_link_wrong_level(tree, tri_in):
    ch = tree.nodes["child"]
    c = int(np.nonzero(ch[0] >= 0)[0][0])
    ch[0, c] = int(tree.level_begin[2])                                   # a node of level 2 under the root
    return ["topology.child_level"]


def m_stack_need_lowered(tree, tri_in):
    tree.header["stack_need"] -= 1
    return ["topology.stack_need"]


def m_leaf_pos_swapped(tree, tri_in):
    tree.leaf_pos[[5, 11]] = tree.leaf_pos[[11, 5]]
    return ["topology.leaf_pos"]


def m_tri48_word_changed(tree, tri_in):
    tree.tri48.view("<u4").reshape(-1, 12)[7, 4] ^= 1
    return ["records.tri48"]


def m_fp16_plane_inwards(tree, tri_in):
    r = int(np.nonzero(tree.coop4["lo_xy"] != tc.EMPTY_COOP[0])[0][3])
    lo_x = np.array([tree.coop4["lo_xy"][r] & 0xFFFF], np.uint16)
    tree.coop4["lo_xy"][r] = (int(tree.coop4["lo_xy"][r]) & 0xFFFF0000) | int(tc._h_inc(lo_x)[0])   # lo.x one fp16 step up
    return ["coop4.box"]


def m_coop16_not_renumbered(tree, tri_in):
    lb = tree.level_begin
    r = int(np.nonzero(tree.coop16["ref"][:16] > 0)[0][0])                # the root's 16 slots: inner references are nodes of level 2
    dense2 = int(lb[1] - lb[0])
    old = int(tree.coop16["ref"][r])
    tree.coop16["ref"][r] = int(lb[2]) + (old - dense2)                   # the 4-wide index, as the per-child array holds it
    assert tree.coop16["ref"][r] != old
    return ["coop16.ref"]


def m_coop16_stale_after_move(tree, tri_in):
    w = tree.tri64.view("<u4").reshape(-1, 16)
    v0 = w[:, 0:3].view("<f4")
    v0[: v0.shape[0] // 2] += np.float32(700.0)                           # half the triangles move; the 16-wide array is not refreshed
    tri_in[w[: v0.shape[0] // 2, 10]] += np.float32(700.0)
    tree.tri48 = w[:, :12].copy().view(tc.TRI48_DT).reshape(-1)
    tree.header["amax"] = np.float32(np.abs(tri_in).max())
    refill(tree, coop16=False)
    return ["coop16.box"]


MUTATIONS = [m_hi_byte_lowered, m_lo_byte_lowered_by_two, m_leaf_ranges_overlap, m_child_link_wrong_level, m_stack_need_lowered,
             m_leaf_pos_swapped, m_tri48_word_changed, m_fp16_plane_inwards, m_coop16_not_renumbered, m_coop16_stale_after_move]


@pytest.mark.parametrize("levels", [3, 4])
@pytest.mark.parametrize("mutation", MUTATIONS, ids=lambda m: m.__name__[2:])
def test_checker_reports_each_fault(mutation, levels):
    tree, tri_in, mat = synth_tree(7 + levels, levels)
    assert run_checks(tree, tri_in, mat) == []
    tri_in = tri_in.copy()
    expected = mutation(tree, tri_in)
    found = run_checks(tree, tri_in, mat)
    for code in expected:
        assert any(s.startswith(code + ":") for s in found), (code, found)


def test_fp16_rounding_restated():
    """h_below / h_above on bit patterns: strictly outside, two steps at most, overflow to infinity beyond 65504"""
    x = np.array([0.0, 1.0, -1.0, 0.1, -0.1, 65504.0, 65519.0, 65520.0, 1e6, -65504.0, -65520.0, -1e6, 6e-8, 1e-9, -1e-9, 2049.0], np.float32)
    lo, hi = tc.h_below(x), tc.h_above(x)
    with np.errstate(over="ignore"):
        near = x.astype(np.float16).view(np.uint16)
    assert np.all(tc._h_val(lo) < x) and np.all(tc._h_val(hi) > x)
    assert np.all(tc._h_val(tc._h_inc(tc._h_inc(lo))) >= x) and np.all(tc._h_val(tc._h_dec(tc._h_dec(hi))) <= x)
    exact = tc._h_val(near) == x
    assert np.array_equal(lo[exact], tc._h_dec(near[exact])) and np.array_equal(hi[exact], tc._h_inc(near[exact]))
    assert hi[7] == 0x7C00 and hi[8] == 0x7C00 and lo[8] == 0x7BFE and lo[11] == 0xFC00 and hi[11] == 0xFBFE
    assert hi[5] == 0x7C00 and lo[9] == 0xFC00                           # one step beyond the largest finite fp16


def test_snapshot_entry_is_exported_but_not_public(pkg):
    lib = pkg._capi.load()
    assert hasattr(lib, "fs_debug_scene_snapshot") and "fs_debug_scene_snapshot" not in pkg._capi.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "fs_debug_scene_snapshot" not in open(os.path.join(root, "include", "frequensee.h")).read()


# ---- GPU: the committed scene ----------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 9, 1023, 1024, 1025, 1500, 5000]
ABSORPTION = np.array([[0.3], [0.5], [0.8]], np.float32)
_levels_seen = {}


def make_soup(T, seed, kind=None, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    kind = kind or ("mixed" if T >= 64 else tc.SOUP_KINDS[seed % len(tc.SOUP_KINDS)])
    tri = tc.soup(kind, T, rng, offset)
    mat = rng.integers(0, 3, T).astype(np.uint16)
    obj = (np.arange(T) // 3 + 5).astype(np.uint32) if T % 2 else None     # with and without actor ids
    return tri, mat, obj


@pytest.fixture(scope="module")
def host_records(pkg):
    """the Tri64 records a host commit of the same triangles holds, in a second context"""
    ctx = pkg.Context(num_bands=1)

    def get(tri, mat, obj):
        ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast=False)
        return tc.fetch(ctx, "tri64").copy()
    yield get
    ctx.close()


def full_check(ctx, tri, mat, obj, host_records, fast, refitted=False, amax=None):
    tree = tc.snapshot(ctx)
    hdr = tree.header
    assert hdr["fast"] == int(bool(fast)) and hdr["refit_pending"] == 0
    assert tree.tri64.shape[0] == tri.shape[0] == hdr["tris"] and tree.nodes.shape[0] == hdr["nodes"]
    assert tree.coop4.shape[0] == 4 * hdr["nodes"] and tree.coop16.shape[0] == 16 * hdr["coop16_nodes"]
    assert hdr["stack_need"] == ctx.stats()["bvh_stack_need"] <= 64
    found = tc.check_all(tree, tri, mat, obj, host_tri64=host_records(tri, mat, obj), device_build=bool(fast), refitted=refitted,
                         amax_expected=np.abs(tri).max() if amax is None else amax)
    assert found == [], "\n".join(found)
    return tree


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["commit", "commit_fast"])
@pytest.mark.parametrize("T", SIZES)
def test_tree_sizes_and_builds(pkg, host_records, T, build):
    """1 and 2 triangles take collapse_kernel's own paths; at 1024 (kCollapseBlock) and below no global PLOC round runs,
    5000 runs several"""
    tri, mat, obj = make_soup(T, T)
    ctx = pkg.Context(num_bands=1)
    ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast=build == "commit_fast")
    tree = full_check(ctx, tri, mat, obj, host_records, fast=build == "commit_fast")
    _levels_seen[(T, build)] = tree.header["levels"]
    ctx.close()


@pytest.mark.gpu
def test_both_level_parities(pkg):
    """coop16_kernel folds two levels into one: a tree with an odd number of levels ends in a level of its own, one with an
    even number does not.  The trees of test_tree_sizes_and_builds (same inputs; rebuilt here if that test did not run in
    this process) have both."""
    for build in ("commit", "commit_fast"):
        for T in SIZES:
            if (T, build) not in _levels_seen:
                tri, mat, obj = make_soup(T, T)
                ctx = pkg.Context(num_bands=1)
                ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast=build == "commit_fast")
                _levels_seen[(T, build)] = tc.fetch(ctx, "header")["levels"]
                ctx.close()
    for build in ("commit", "commit_fast"):
        parities = {_levels_seen[(T, build)] % 2 for T in SIZES}
        assert parities == {0, 1}, (build, {T: _levels_seen[(T, build)] for T in SIZES})


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["commit", "commit_fast"])
@pytest.mark.parametrize("offset,infinite", [((20000.0, -3000.0, 500.0), False), ((70000.0, -72000.0, 300.0), True)])
def test_tree_large_coordinates(pkg, host_records, offset, infinite, build):
    """beyond kCoopMaxCoordinate (16384) the cooperative arrays are not used but still written; beyond 65504 their planes
    are infinite"""
    tri, mat, obj = make_soup(1500, 31, offset=offset)
    assert np.abs(tri).max() > 16384
    ctx = pkg.Context(num_bands=1)
    ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast=build == "commit_fast")
    tree = full_check(ctx, tri, mat, obj, host_records, fast=build == "commit_fast")
    assert tc.has_infinite_planes(tree.coop4) == infinite and tc.has_infinite_planes(tree.coop16) == infinite
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["commit", "commit_fast"])
def test_tree_moving_geometry(pkg, host_records, build):
    T = 1500
    fast = build == "commit_fast"
    tri, mat, obj = make_soup(T, 41)
    rng = np.random.default_rng(43)
    ctx = pkg.Context(num_bands=1)
    ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast=fast)
    before = full_check(ctx, tri, mat, obj, host_records, fast=fast)
    cur = tri.copy()
    amax = np.float32(np.abs(cur).max())
    zero = tc.soup("zero_area", 60, rng)
    zero[3::4] = zero[1::4]                                               # (every triangle of this part without area)
    steps = [("middle range", 400, cur[400:900] + rng.normal(0, 40, (500, 3, 3)).astype(np.float32)),
             ("last triangle", T - 1, cur[T - 1:] + np.float32(25.0)),
             ("all", 0, tc.soup("mixed", T, rng)),
             ("prop far out", 100, tc.soup("uniform", 60, rng, offset=(52000.0, 100.0, -48000.0))),
             ("prop back", 100, tc.soup("uniform", 60, rng)),
             ("zero area", 200, zero)]
    pads = [tc.refit_pad(before.header)]
    for name, first, new in steps:
        ctx.update_triangles(first, new)
        cur[first:first + new.shape[0]] = new
        amax = max(amax, np.float32(np.abs(new).max()))
        for _ in range(2):                                                # the snapshot itself runs no refit
            hdr = tc.fetch(ctx, "header")
            assert hdr["refit_pending"] == 1, name
        mid = tc.snapshot(ctx)
        assert tc.check_records(mid, cur, mat, obj) == [], name           # the records are new already ...
        assert mid.nodes.tobytes() == before.nodes.tobytes(), name        # ... the boxes still old
        assert mid.coop4.tobytes() == before.coop4.tobytes() and mid.coop16.tobytes() == before.coop16.tobytes(), name
        ctx.refit()
        after = full_check(ctx, cur, mat, obj, host_records, fast=fast, refitted=True, amax=amax)
        assert np.array_equal(after.nodes["child"], before.nodes["child"]), name
        assert np.array_equal(tc._used(after.nodes), tc._used(before.nodes)), name   # used slots stay used, empty ones empty
        assert np.array_equal(after.leaf_pos, before.leaf_pos) and np.array_equal(after.level_begin, before.level_begin), name
        pads.append(tc.refit_pad(after.header))
        before = after
    assert all(b >= a for a, b in zip(pads, pads[1:])), pads               # the padding never shrinks ...
    assert pads[4] > pads[3] and pads[5] == pads[4], pads                  # ... and grew with the prop far outside the old bounds
    ctx.close()


@pytest.mark.gpu
def test_tree_reregistration(pkg, host_records):
    """a fast commit keeps its arrays for the next registration: a smaller scene committed into them holds nothing of the first"""
    ctx = pkg.Context(num_bands=1)
    tri, mat, obj = make_soup(5000, 51)
    ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast=True)
    first = full_check(ctx, tri, mat, obj, host_records, fast=True)
    tri2, mat2, obj2 = make_soup(1500, 52, offset=(300.0, -200.0, 100.0))
    ctx.set_scene(tri2, mat2, ABSORPTION, object_ids=obj2, fast=True)
    second = full_check(ctx, tri2, mat2, obj2, host_records, fast=True)
    assert second.tri64.shape[0] == 1500 and second.nodes.shape[0] < first.nodes.shape[0]
    assert second.leaf_pos.shape[0] == 1500 and second.node_box.shape[0] == second.nodes.shape[0]
    ctx.close()


@pytest.mark.gpu
def test_tree_progressive_commit(pkg, host_records):
    """the device-built tree at once, the host's SAH tree after refine_wait"""
    tri, mat, obj = make_soup(5000, 61)
    ctx = pkg.Context(num_bands=1)
    ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast="progressive")
    quick = full_check(ctx, tri, mat, obj, host_records, fast=True)
    ctx.refine_wait()
    assert not ctx.refine_pending()
    fine = full_check(ctx, tri, mat, obj, host_records, fast=False)
    assert fine.nodes.tobytes() != quick.nodes.tobytes()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 1500])
def test_tree_host_build_refit_without_a_move(pkg, host_records, T):
    """fs_scene_refit on a host-built tree nobody moved: the boxes now come from the records (check d)"""
    tri, mat, obj = make_soup(T, 71)
    ctx = pkg.Context(num_bands=1)
    ctx.set_scene(tri, mat, ABSORPTION, object_ids=obj, fast=False)
    ctx.refit()
    full_check(ctx, tri, mat, obj, host_records, fast=False, refitted=True)
    ctx.close()
