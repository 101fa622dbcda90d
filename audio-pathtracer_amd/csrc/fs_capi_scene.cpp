// fs_capi_scene.cpp — geometry and material registration, tree commits (host SAH, device Morton, progressive),
// moving geometry (C ABI: include/frequensee.h; RegisterGeometry / UAcousticMaterial, ARTS.h:99-100, MAT.h:22-33).
#include "fs_context.hpp"

static int update_triangles(fs_context* ctx, int32_t first, int32_t count, const float* xyz, bool new_rest);

namespace fsi {

// A background build that is no longer wanted: the builder polls the flag and gives up; the thread itself is joined by
// fs_context_destroy (join_refine_threads) — never left running inside a library that may be unloaded.
void cancel_refine(fs_context* ctx) {
    if (ctx->refine) ctx->refine->cancel.store(true, std::memory_order_relaxed);
    ctx->refine.reset();
    ctx->moved_since_refine = false;
}
void wait_refine(const std::shared_ptr<RefineJob>& j) {
    std::unique_lock<std::mutex> l(j->mu);
    j->cv.wait(l, [&] { return j->done; });
}
void join_refine_threads(fs_context* ctx) {
    for (std::thread& t : ctx->refine_threads)
        if (t.joinable()) t.join();
    ctx->refine_threads.clear();
}

// ---- fs_scene_set_object_transforms: the host side of the rest pose ---------------------------------------------------
// one vertex by a row-major 3 x 4 matrix, every operation rounded (this file is built with -ffp-contract=off, as
// transform_objects_kernel is): ((r0 x + r1 y) + r2 z) + t
static inline void transform_vertex(const float* a, const float* r, float* w) {
    const float x = r[0], y = r[1], z = r[2];
    for (int k = 0; k < 3; ++k) w[k] = ((a[4 * k] * x + a[4 * k + 1] * y) + a[4 * k + 2] * z) + a[4 * k + 3];
}

// h_xyz = the world positions: the objects moved by transform since it was last brought up to date get their newest matrix
// applied to their rest positions (what the device records already hold)
void sync_world_positions(fs_context* ctx) {
    ObjectMoves* mv = ctx->moves;
    if (!mv || mv->stale_list.empty()) return;
    for (uint32_t slot : mv->stale_list) {
        const float* a = mv->m.data() + 12 * (size_t)slot;
        for (uint32_t j = mv->off[slot]; j < mv->off[slot + 1]; ++j) {
            const size_t t = mv->idx[j];
            for (int v = 0; v < 3; ++v) transform_vertex(a, mv->rest.data() + 9 * t + 3 * v, ctx->h_xyz.data() + 9 * t + 3 * v);
        }
        mv->stale[slot] = 0;
    }
    mv->stale_list.clear();
}

// the largest |coordinate| transform_objects_kernel has written, folded into ctx->amax where the padding is computed or
// reported: waits for the one 4-byte copy enqueued behind the newest kernel
static hipError_t fold_moved_amax(fs_context* ctx) {
    ObjectMoves* mv = ctx->moves;
    if (!mv || !mv->amax_pending) return hipSuccess;
    const hipError_t e = hipEventSynchronize(mv->ev_amax);
    if (e != hipSuccess) return e;
    float v;
    std::memcpy(&v, mv->h_amax, sizeof(float));
    ctx->amax = std::max(ctx->amax, v);
    mv->amax_pending = false;
    return hipSuccess;
}

// every commit: the lists and the device copies describe the tree that has just been replaced (the rest pose stays)
static void object_moves_after_commit(fs_context* ctx) {
    ObjectMoves* mv = ctx->moves;
    if (!mv) return;
    mv->lists_valid = false;
    mv->on_device = false;
    mv->amax_pending = false;    // (the commit has drained the stream and taken amax from h_xyz)
    mv->stale_list.clear();
    if (mv->d_amax) (void)hipMemsetAsync(mv->d_amax, 0, sizeof(uint32_t), ctx->stream);
}

void free_object_moves(fs_context* ctx) {
    ObjectMoves* mv = ctx->moves;
    if (!mv) return;
    if (mv->d_rest) (void)hipFree(mv->d_rest);
    if (mv->d_idx) (void)hipFree(mv->d_idx);
    if (mv->d_amax) (void)hipFree(mv->d_amax);
    if (mv->h_amax) (void)hipHostFree(mv->h_amax);
    if (mv->ev_amax) (void)hipEventDestroy(mv->ev_amax);
    for (ObjectMoves::Set& st : mv->set) {
        if (st.h) (void)hipHostFree(st.h);
        if (st.d) (void)hipFree(st.d);
        if (st.ev) (void)hipEventDestroy(st.ev);
    }
    delete mv;
    ctx->moves = nullptr;
}

// fs_scene_commit_progressive: once the background build has finished, the next call that traces anything swaps its tree
// in — held frames finish first (they were traced through the old tree's arrays), the stream drains, the records are
// uploaded; triangles moved since the snapshot get their current positions and a refit.
int maybe_install_refined(fs_context* ctx) {
    if (!ctx->refine) return FS_OK;
    std::shared_ptr<RefineJob> j = ctx->refine;
    { std::lock_guard<std::mutex> l(j->mu); if (!j->done) return FS_OK; }
    const bool moved = ctx->moved_since_refine;
    ctx->refine.reset();
    ctx->moved_since_refine = false;
    if (j->T != ctx->T || !ctx->committed) return FS_OK;
    ctx->prebuilt = &j->bvh;
    const uint64_t gen = ctx->scene_gen;   // a better tree over the same triangles: no change of the scene (fs_pathing_info)
    int rc = fs_scene_commit(ctx);
    ctx->prebuilt = nullptr;
    if (!rc && moved) {   // (the commit has brought h_xyz up to the world positions; the rest pose is not touched)
        const std::vector<float> now = ctx->h_xyz;
        rc = update_triangles(ctx, 0, ctx->T, now.data(), false);
    }
    ctx->scene_gen = gen;
    return rc;
}

}  // namespace fsi

extern "C" {

// ---- scene -----------------------------------------------------------------------------------------
int fs_scene_set_triangles(fs_context* ctx, const float* xyz, const uint16_t* mat_id, int32_t T) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (T < 0 || (T > 0 && !xyz)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad triangle array");
    if (T > (1 << 28)) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "too many triangles");
    for (size_t i = 0; i < 9 * (size_t)T; ++i)
        if (!std::isfinite(xyz[i])) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
    cancel_refine(ctx);   // a background build of the previous triangle set is of no use any more
    if (ctx->moves) {     // a new rest pose: h_xyz itself until the next fs_scene_set_object_transforms
        ctx->moves->rest.clear(); ctx->moves->rest_amax = 0.0;
        ctx->moves->stale_list.clear(); ctx->moves->lists_valid = false;
    }
    ctx->h_xyz.assign(xyz, xyz + 9 * (size_t)T);
    if (mat_id) ctx->h_mat.assign(mat_id, mat_id + T);
    else ctx->h_mat.assign((size_t)T, (uint16_t)FS_NO_MATERIAL);
    ctx->T = T;
    ctx->committed = false;
    return FS_OK;
}

int fs_scene_set_materials(fs_context* ctx, const float* absorption, const float* transmission,
                           const float* scattering, int32_t M, int32_t B) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (M < 0 || (M > 0 && !absorption) || M >= (int32_t)FS_NO_MATERIAL)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "bad material table");
    if (B != ctx->cfg.num_bands) return ctx->fail(FS_ERR_SIZE_MISMATCH, "material bands != context num_bands");
    size_t n = (size_t)M * (size_t)B;
    ctx->h_absorption.assign(absorption, absorption + n);
    if (transmission) ctx->h_transmission.assign(transmission, transmission + n); else ctx->h_transmission.clear();
    if (scattering) ctx->h_scattering.assign(scattering, scattering + n); else ctx->h_scattering.clear();
    ctx->M = M;
    ctx->committed = false;
    return FS_OK;
}

// the material table of a committed scene: absorption [M][B] | lobe gains [M][3][B] | lobe probabilities [M][3]
static int upload_materials(fs_context* ctx) {
    const size_t mb = ctx->h_absorption.size() * sizeof(float);
    if (mb) {
        // absorption [M][B] | lobe gains [M][3][B] | lobe probabilities [M][3] (FS_FLAG_MATERIAL_LOBES).  The split is
        // the per-bin rule of ApplyMaterialFD (MaterialAcousticProcessor.cpp:51-72) per band: Refl = 1 - alpha, tau
        // clamped to Refl + tau <= 1, diffuse Refl sigma, specular Refl (1 - sigma), transmitted tau; a lobe is
        // picked with the band mean of its gain over the sum of the three.  No arrays: tau = 0, sigma = 1.
        const int B = ctx->cfg.num_bands, M = ctx->M;
        std::vector<float> table(ctx->h_absorption);
        table.resize((size_t)M * B + (size_t)M * 3 * B + (size_t)M * 3, 0.f);
        float* gain = table.data() + (size_t)M * B;
        float* prob = gain + (size_t)M * 3 * B;
        const bool has_t = ctx->h_transmission.size() == (size_t)M * B, has_s = ctx->h_scattering.size() == (size_t)M * B;
        for (int m = 0; m < M; ++m) {
            float sum[3] = {0.f, 0.f, 0.f};
            for (int b = 0; b < B; ++b) {
                const float alpha = ctx->h_absorption[(size_t)m * B + b];
                float tau = has_t ? ctx->h_transmission[(size_t)m * B + b] : 0.0f;
                const float sigma = has_s ? ctx->h_scattering[(size_t)m * B + b] : 1.0f;
                const float refl = 1.0f - alpha;
                if (refl + tau > 1.0f) tau = 1.0f - refl;
                float g[3] = {refl * sigma, refl * (1.0f - sigma), tau};
                for (int l = 0; l < 3; ++l) {
                    if (!(g[l] > 0.0f)) g[l] = 0.0f;
                    gain[((size_t)m * 3 + l) * B + b] = g[l];
                    sum[l] += g[l];
                }
            }
            float mean[3], tot = 0.0f;
            for (int l = 0; l < 3; ++l) { mean[l] = sum[l] / (float)B; tot += mean[l]; }
            for (int l = 0; l < 3; ++l) prob[(size_t)m * 3 + l] = tot > 0.0f ? mean[l] / tot : (l == 0 ? 1.0f : 0.0f);
        }
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_absorption, table.size() * sizeof(float)));
        FS_HIP(ctx, hipMemcpy(ctx->d_absorption, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return FS_OK;
}

// the kernels' view of the triangle records (Tri48 + normals), derived on the device from the authoring records; `cap`
// = records the arrays must have room for (the fast commit keeps its arrays for the next registration)
static int pack_scene(fs_context* ctx, size_t count, size_t cap) {
    if (!ctx->d_tris48) {
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_tris48, std::max<size_t>(cap, 1) * sizeof(Tri48)));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_tri_nrm, std::max<size_t>(cap, 1) * sizeof(float4)));
    }
    launch_pack_triangles(ctx->d_tris, (int)count, ctx->d_tris48, ctx->d_tri_nrm, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    return FS_OK;
}

// what every kind of commit ends with: the kernels' view of the scene and the stats
// the cooperative traversal's records, derived from the node array as it stands in the stream (behind an upload, a device
// build's refit, a refit of moved triangles)
static int refresh_coop_nodes(fs_context* ctx, bool topology_changed) {
    const size_t n = ctx->bvh.nodes.size();
    const int levels = (int)ctx->bvh.level_begin.size() - 1;
    ctx->coop_info = CoopInfo{};
    ctx->scene.coop_info = &ctx->coop_info;
    if (n == 0 || levels < 1 || levels > kMaxBuildLevels) return FS_OK;
    if (n > ctx->coop_cap) {
        if (ctx->d_coop) { FS_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->d_coop); }
        ctx->d_coop = nullptr; ctx->coop_cap = 0;
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_coop, sizeof(CoopChild) * 4 * n));
        ctx->coop_cap = n;
    }
    if (topology_changed || !ctx->d_coop_levels) {   // the level table and the dense numbering of the even levels (a refit keeps both)
        std::vector<int32_t> tab(2 * (size_t)(kMaxBuildLevels + 2), -1);
        int32_t n16 = 0;
        for (int l = 0; l <= levels; ++l) tab[(size_t)l] = ctx->bvh.level_begin[(size_t)l];
        for (int l = 0; l < levels; ++l) {
            if (l & 1) continue;
            tab[(size_t)(kMaxBuildLevels + 2) + (size_t)l] = n16;
            n16 += ctx->bvh.level_begin[(size_t)l + 1] - ctx->bvh.level_begin[(size_t)l];
        }
        if (!ctx->d_coop_levels) FS_HIP(ctx, hipMalloc((void**)&ctx->d_coop_levels, sizeof(int32_t) * tab.size()));
        FS_HIP(ctx, hipMemcpyAsync(ctx->d_coop_levels, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (tab is a local; commits drain the stream anyway)
        ctx->coop16_nodes = n16; ctx->coop_levels = levels;
    }
    if ((size_t)ctx->coop16_nodes > ctx->coop16_cap) {
        if (ctx->d_coop16) { FS_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->d_coop16); }
        ctx->d_coop16 = nullptr; ctx->coop16_cap = 0;
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_coop16, sizeof(CoopChild) * 16 * (size_t)ctx->coop16_nodes));
        ctx->coop16_cap = (size_t)ctx->coop16_nodes;
    }
    launch_coop_nodes(ctx->d_nodes, (int)n, ctx->d_coop, ctx->stream);
    launch_coop16(ctx->d_coop, ctx->d_coop_levels, ctx->d_coop_levels + (kMaxBuildLevels + 2), ctx->coop_levels, ctx->coop16_nodes, ctx->d_coop16, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    // one-node-at-a-time descents: 15 new entries per 16-wide level at most; the 4-wide tree's bound is the builder's (+ the popped node's four)
    ctx->coop_info.wide16 = CoopView{ctx->d_coop16, 0, ctx->coop16_nodes, 4, (int16_t)(15 * ((ctx->coop_levels + 1) / 2) + 1)};
    ctx->coop_info.wide4 = CoopView{ctx->d_coop, 0, (int32_t)n, 2, (int16_t)(std::max(ctx->bvh.stack_need, 2) + 4)};
    // The cooperative records hold ABSOLUTE world coordinates rounded outwards to fp16 (fs_refit.hip): conservative at any size,
    // but the fp16 ulp is 8 units at 10^4 and 16 - 32 at a few 10^4 (beyond 65 504 the planes are infinite): on a large map the
    // boxes stop culling and the search degenerates silently.  Such scenes take the lane-private traversal (node-relative 8-bit
    // grids) for their small frames instead: coop_view finds no usable record array.
    if (ctx->amax > kCoopMaxCoordinate) { ctx->coop_info.wide16.rec = nullptr; ctx->coop_info.wide4.rec = nullptr; }
    static const bool dbg_info = std::getenv("FS_DEBUG_SCENE_INFO") != nullptr;   // (what DESIGN.md quotes)
    if (dbg_info)
        std::fprintf(stderr, "[frequensee] tree: %zu 4-wide nodes in %d levels -> %d 16-wide nodes\n", n, levels, ctx->coop16_nodes);
    return FS_OK;
}

// The 48-byte node view of the chip-filling frame kernel (fs_internal.hpp: ViewRec), called wherever refresh_coop_nodes is
// (behind it: that one resets coop_info).  The layout follows the topology: computed behind a commit and kept across refits;
// the contents are re-derived from the arrays as they stand in the stream.  A scene whose view does not fit the request's
// offsets, or one of whose grid steps is no power of two, stays without a view: launch_frame takes another route for it.
// The only wait is the commit's (a refit adds none): the fill's verdict is read once, where the stream is drained anyway.
static int refresh_node_view(fs_context* ctx, bool topology_changed) {
    const size_t n = ctx->bvh.nodes.size(), T = (size_t)ctx->T;
    ctx->coop_info.view = NodeView{};
    ctx->scene.coop_info = &ctx->coop_info;
    if (topology_changed) ctx->view_ok = false;
    if (n == 0 || ctx->view_off || !node_view_fits(n, T)) { ctx->view_ok = false; return FS_OK; }
    if (!topology_changed && !ctx->view_ok) return FS_OK;
    if (topology_changed) {
        if (n > ctx->view_cap_nodes || T > ctx->view_cap_tris) {
            FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            for (void* v : {(void*)ctx->d_view, (void*)ctx->d_view_nrm, (void*)ctx->d_view_scan, (void*)ctx->d_view_of_node, (void*)ctx->d_view_of_leaf})
                if (v) (void)hipFree(v);
            ctx->d_view = nullptr; ctx->d_view_nrm = nullptr; ctx->d_view_scan = nullptr; ctx->d_view_of_node = nullptr; ctx->d_view_of_leaf = nullptr;
            ctx->view_cap_nodes = 0; ctx->view_cap_tris = 0;
            const size_t cn = std::max(n, ctx->fast_cap_tris), ct = std::max(T, ctx->fast_cap_tris);   // (a fast commit keeps room for the next registration)
            FS_HIP(ctx, hipMalloc((void**)&ctx->d_view, sizeof(ViewRec) * (cn + ct)));
            FS_HIP(ctx, hipMalloc((void**)&ctx->d_view_nrm, sizeof(float4) * (cn + ct)));
            FS_HIP(ctx, hipMalloc((void**)&ctx->d_view_scan, sizeof(uint32_t) * (cn + 1)));
            FS_HIP(ctx, hipMalloc((void**)&ctx->d_view_of_node, sizeof(uint32_t) * cn));
            FS_HIP(ctx, hipMalloc((void**)&ctx->d_view_of_leaf, sizeof(uint32_t) * std::max<size_t>(ct, 1)));
            ctx->view_cap_nodes = cn; ctx->view_cap_tris = ct;
        }
        if (!ctx->d_view_bad) FS_HIP(ctx, hipMalloc((void**)&ctx->d_view_bad, sizeof(uint32_t)));
        FS_HIP(ctx, hipMemsetAsync(ctx->d_view_bad, 0, sizeof(uint32_t), ctx->stream));
        FS_HIP(ctx, hipMemsetAsync(ctx->d_view_nrm, 0, sizeof(float4) * (n + T), ctx->stream));   // (node slots: unused, but handed out by the snapshot)
        launch_node_view_layout(ctx->d_nodes, (int)n, (int)T, ctx->d_view_scan, ctx->d_view_of_node, ctx->d_view_of_leaf, ctx->stream);
    }
    launch_node_view_fill(ctx->d_nodes, (int)n, ctx->d_tris48, ctx->d_tri_nrm, (int)T, ctx->d_view_scan, ctx->d_view_of_node, ctx->d_view_of_leaf,
                          ctx->d_view, ctx->d_view_nrm, ctx->d_view_bad, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    if (topology_changed) {   // every record placed exactly once <=> the blocks hold nodes - 1 + triangles records and none was reported
        uint32_t verdict[2] = {1u, 0u};
        FS_HIP(ctx, hipMemcpyAsync(&verdict[0], ctx->d_view_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(ctx, hipMemcpyAsync(&verdict[1], ctx->d_view_scan + n, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->view_ok = verdict[0] == 0u && (size_t)verdict[1] + 1 == n + T;
    }
    if (ctx->view_ok) ctx->coop_info.view = NodeView{ctx->d_view, ctx->d_view_nrm};
    return FS_OK;
}
// what fs_scene_update_triangles and fs_scene_set_object_transforms hand their kernels: the view's copies follow in place
static ViewTris view_tris(const fs_context* ctx) {
    return ctx->view_ok ? ViewTris{ctx->d_view, ctx->d_view_nrm, ctx->d_view_of_leaf} : ViewTris{nullptr, nullptr, nullptr};
}

static int finish_commit(fs_context* ctx, size_t scene_bytes) {
    // the traversal's requests carry 32-bit byte offsets into the node and triangle records (DeviceScene, fs_internal.hpp)
    if ((uint64_t)ctx->bvh.nodes.size() * sizeof(NodeQ4) > 0xFFFFFFFFull || (uint64_t)ctx->T * sizeof(Tri48) > 0xFFFFFFFFull)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "scene too large: node or triangle records exceed 4 GiB");
    object_moves_after_commit(ctx);
    ctx->amax = 0.f;
    for (float v : ctx->h_xyz) ctx->amax = std::max(ctx->amax, std::fabs(v));
    ctx->scene.nodes = ctx->d_nodes;
    ctx->scene.tris = ctx->d_tris48;
    ctx->scene.tri_nrm = ctx->d_tri_nrm;
    ctx->scene.absorption = ctx->d_absorption;
    ctx->scene.lobe_gain = ctx->d_absorption ? ctx->d_absorption + (size_t)ctx->M * ctx->cfg.num_bands : nullptr;
    ctx->scene.lobe_prob = ctx->d_absorption ? ctx->scene.lobe_gain + (size_t)ctx->M * 3 * ctx->cfg.num_bands : nullptr;
    ctx->scene.num_nodes = (int32_t)ctx->bvh.nodes.size();
    ctx->scene.num_tris = ctx->T;
    ctx->scene.num_materials = ctx->M;
    // LDS rows of the traversal stack: the tree's worst case + 1 if that is at most stack_rows_cap + 1 rows; else
    // stack_rows_cap rows + one row of counters, and a deep store in HBM for the rare lane that needs more
    // (fs_internal.hpp: DeviceScene.deep).  The bounded stack is what lets four workgroups share a CU.
    const int worst = std::max(ctx->bvh.stack_need, 2) + kStackSlack;
    int deep_rows = 0;
    if (worst <= ctx->stack_rows_cap + 1) {
        ctx->scene.stack_rows = worst; ctx->scene.stack_limit = worst; ctx->scene.stack_attn = 0x7FFFFFFFu;
    } else {
        ctx->scene.stack_rows = ctx->stack_rows_cap + 1; ctx->scene.stack_limit = ctx->stack_rows_cap;
        ctx->scene.stack_attn = (uint32_t)(ctx->stack_rows_cap - 4);
        deep_rows = ((worst + kDeepChunk - 1) / kDeepChunk) * kDeepChunk + kDeepChunk;
    }
    if (deep_rows != ctx->deep.rows) {   // (every commit has drained the stream: nothing reads the old store any more)
        if (ctx->deep.buf) (void)hipFree(ctx->deep.buf);
        for (int32_t* b : ctx->deep.retired) (void)hipFree(b);
        ctx->deep = DeepStore{};
        ctx->deep.rows = deep_rows;
    }
    ctx->scene.stack_worst = traversal_lds_bytes(worst, ctx->cfg.num_bands, ctx->num_bins) <= ctx->lds_limit ? worst : 0;
    ctx->scene.deep = nullptr; ctx->scene.deep_lanes = 0;
    ctx->scene.deep_owner = &ctx->deep;
    ctx->stats.bvh_nodes = (uint32_t)ctx->bvh.nodes.size();
    ctx->stats.triangles = (uint32_t)ctx->T;
    ctx->stats.bvh_stack_need = (uint32_t)ctx->bvh.stack_need;
    ctx->stats.bvh_depth = (uint32_t)ctx->bvh.max_depth;
    ctx->stats.scene_bytes = scene_bytes;
    ctx->scene.coop_info = nullptr;
    { const int cr = refresh_coop_nodes(ctx, true); if (cr) return cr; }
    { const int vr = refresh_node_view(ctx, true); if (vr) return vr; }
    ctx->committed = true;
    ctx->scene_gen += 1;
    return FS_OK;
}

int fs_scene_commit(fs_context* ctx) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    sync_world_positions(ctx);   // objects moved by transform: the tree is built over where they are now
    if (!ctx->prebuilt) cancel_refine(ctx);
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_scene(ctx);
    ctx->fast_cap_tris = 0;
    // With a communicator attached rank 0 alone builds the acceleration structure and broadcasts it; the
    // other ranks only hold the triangles for later fs_scene_update_triangles bookkeeping.
    RcclApi* ra = ctx->comm ? rccl() : nullptr;
    if (ctx->comm && !ra) return ctx->fail(FS_ERR_COMM, "communicator attached but librccl is not loadable");
    const bool bcast = ra != nullptr;
    const bool root = !bcast || ctx->cfg.rank == 0;
    size_t n_nodes = 0, n_tris = 0, n_leaf = 0, n_lvl = 0;
    if (root) {
        if (ctx->prebuilt) ctx->bvh = std::move(*ctx->prebuilt);   // the background build of fs_scene_commit_progressive
        else
            build_bvh(ctx->h_xyz.data(), ctx->h_mat.data(),
                      ctx->h_obj.size() == (size_t)ctx->T && ctx->T > 0 ? ctx->h_obj.data() : nullptr, ctx->T, ctx->bvh);
        n_nodes = ctx->bvh.nodes.size(); n_tris = ctx->bvh.tris.size();
        n_leaf = ctx->bvh.leaf_pos.size(); n_lvl = ctx->bvh.level_begin.size();
    }
    if (bcast) {   // header first: sizes, stack bound, box padding
        int32_t hdr[8] = {(int32_t)n_nodes, (int32_t)n_tris, (int32_t)n_leaf, (int32_t)n_lvl, ctx->bvh.stack_need,
                          ctx->bvh.max_depth, 0, ctx->T};
        std::memcpy(&hdr[6], &ctx->bvh.pad, sizeof(float));
        int32_t* d_hdr = nullptr;
        FS_HIP(ctx, hipMalloc((void**)&d_hdr, sizeof(hdr)));
        if (root) FS_HIP(ctx, hipMemcpyAsync(d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, ctx->stream));
        ncclResult_t r = ra->Broadcast(d_hdr, d_hdr, 8, ncclInt32, 0, ctx->comm, ctx->stream);
        hipError_t e = hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_hdr);
        if (r != ncclSuccess) return nccl_fail(ctx, r, "ncclBroadcast(scene header)");
        if (e != hipSuccess) return ctx->hip_fail(e, "scene header");
        if (hdr[7] != ctx->T) return ctx->fail(FS_ERR_SIZE_MISMATCH, "fs_scene_commit: rank 0 committed a different number of triangles");
        if (!root) {
            n_nodes = (size_t)hdr[0]; n_tris = (size_t)hdr[1]; n_leaf = (size_t)hdr[2]; n_lvl = (size_t)hdr[3];
            ctx->bvh = HostBVH{};
            ctx->bvh.stack_need = hdr[4]; ctx->bvh.max_depth = hdr[5];
            std::memcpy(&ctx->bvh.pad, &hdr[6], sizeof(float));
            ctx->bvh.nodes.resize(n_nodes); ctx->bvh.tris.resize(n_tris);   // sizes only; the records live on the device
            ctx->bvh.level_begin.assign(n_lvl, 0);
        }
    }
    if (ctx->bvh.stack_need > kStackDepth) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "BVH needs a deeper traversal stack");
    {   // the traversal kernels keep stack + energy histogram window + work-sharing area in LDS: fail here, with a
        // message, rather than with a launch error on every frame
        const size_t need = traversal_lds_bytes(std::min(std::max(ctx->bvh.stack_need, 2) + kStackSlack, ctx->stack_rows_cap + 1), ctx->cfg.num_bands, ctx->num_bins);
        if (need > ctx->lds_limit)
            return ctx->fail(FS_ERR_INVALID_ARGUMENT, "scene + energy histogram need " + std::to_string(need) +
                             " B of LDS per workgroup, the device offers " + std::to_string(ctx->lds_limit));
    }
    size_t nb = n_nodes * sizeof(NodeQ4), tb = n_tris * sizeof(Tri64);
    size_t mb = ctx->h_absorption.size() * sizeof(float);
    if (nb) {
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_nodes, nb));
        if (root) FS_HIP(ctx, hipMemcpyAsync(ctx->d_nodes, ctx->bvh.nodes.data(), nb, hipMemcpyHostToDevice, ctx->stream));
        if (bcast) FS_NCCL(ctx, ra->Broadcast(ctx->d_nodes, ctx->d_nodes, nb, ncclUint8, 0, ctx->comm, ctx->stream));
    }
    if (tb) {
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_tris, tb));
        if (root) FS_HIP(ctx, hipMemcpyAsync(ctx->d_tris, ctx->bvh.tris.data(), tb, hipMemcpyHostToDevice, ctx->stream));
        if (bcast) FS_NCCL(ctx, ra->Broadcast(ctx->d_tris, ctx->d_tris, tb, ncclUint8, 0, ctx->comm, ctx->stream));
    }
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    { int mr = upload_materials(ctx); if (mr) return mr; }
    if (tb) {   // refit support: leaf positions, level table and the bounds scratch
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_leaf_pos, sizeof(uint32_t) * std::max<size_t>(n_leaf, 1)));
        if (root) FS_HIP(ctx, hipMemcpyAsync(ctx->d_leaf_pos, ctx->bvh.leaf_pos.data(), sizeof(uint32_t) * n_leaf,
                                             hipMemcpyHostToDevice, ctx->stream));
        if (bcast) {
            FS_NCCL(ctx, ra->Broadcast(ctx->d_leaf_pos, ctx->d_leaf_pos, n_leaf, ncclUint32, 0, ctx->comm, ctx->stream));
            int32_t* d_lvl = nullptr;   // the level table is host data (one refit launch per level): through a device bounce buffer
            FS_HIP(ctx, hipMalloc((void**)&d_lvl, sizeof(int32_t) * std::max<size_t>(n_lvl, 1)));
            if (root) FS_HIP(ctx, hipMemcpyAsync(d_lvl, ctx->bvh.level_begin.data(), sizeof(int32_t) * n_lvl, hipMemcpyHostToDevice, ctx->stream));
            ncclResult_t r = ra->Broadcast(d_lvl, d_lvl, n_lvl, ncclInt32, 0, ctx->comm, ctx->stream);
            hipError_t e = hipSuccess;
            if (!root) e = hipMemcpyAsync(ctx->bvh.level_begin.data(), d_lvl, sizeof(int32_t) * n_lvl, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            (void)hipFree(d_lvl);
            if (r != ncclSuccess) return nccl_fail(ctx, r, "ncclBroadcast(level table)");
            if (e != hipSuccess) return ctx->hip_fail(e, "level table");
        }
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_node_box, sizeof(float4) * 2 * std::max<size_t>(n_nodes, 1)));
        // (scratch of the refit, but fs_debug_scene_snapshot hands it out: defined — zero — until the first refit writes it,
        // not whatever the allocation held before)
        FS_HIP(ctx, hipMemsetAsync(ctx->d_node_box, 0, sizeof(float4) * 2 * std::max<size_t>(n_nodes, 1), ctx->stream));
    }
    if (tb) { const int pr = pack_scene(ctx, n_tris, n_tris); if (pr) return pr; }
    return finish_commit(ctx, nb + n_tris * (sizeof(Tri48) + sizeof(float4)) + mb);
}

// RegisterGeometry / UnregisterGeometry at run time (ARTS.h:99-100): a changed triangle set needs a new tree NOW.
// The whole build runs on the device (fs_build.hip) behind one upload of the triangles; the host only reads back the
// level table and the stack bound.  Falls back to the host build when the Morton tree comes out too deep.
int fs_scene_commit_fast(fs_context* ctx) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    sync_world_positions(ctx);   // objects moved by transform: the tree is built over where they are now
    cancel_refine(ctx);
    if (ctx->T < 1 || ctx->comm) return fs_scene_commit(ctx);   // empty scene / sharded run: the one build rank 0 broadcasts
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int T = ctx->T;
    const size_t n = (size_t)T;
    const bool reuse = ctx->fast_cap_tris >= n && ctx->d_nodes && ctx->d_tris && ctx->d_leaf_pos && ctx->d_node_box;
    if (!reuse) { free_scene(ctx); ctx->fast_cap_tris = 0; }
    else {   // keep the four arrays of the previous fast commit, drop the rest of the old scene
        if (ctx->d_absorption) (void)hipFree(ctx->d_absorption);
        ctx->d_absorption = nullptr;
        ctx->refit_pending = false;
        ctx->committed = false;
    }
    // inputs + scratch in one grow-only device block (hipMalloc costs more than the build)
    const size_t in_bytes = ((sizeof(float) * 9 * n + 255) & ~(size_t)255) + ((sizeof(uint16_t) * n + 255) & ~(size_t)255) +
                            ((sizeof(uint32_t) * n + 255) & ~(size_t)255) + 256;
    const size_t scratch_bytes = device_build_scratch_bytes(T);
    if (in_bytes + scratch_bytes > ctx->build_cap) {
        if (ctx->d_build) (void)hipFree(ctx->d_build);
        ctx->d_build = nullptr; ctx->build_cap = 0;
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_build, in_bytes + scratch_bytes));
        ctx->build_cap = in_bytes + scratch_bytes;
    }
    char* q = ctx->d_build;
    float* d_xyz = reinterpret_cast<float*>(q); q += (sizeof(float) * 9 * n + 255) & ~(size_t)255;
    uint16_t* d_mat = reinterpret_cast<uint16_t*>(q); q += (sizeof(uint16_t) * n + 255) & ~(size_t)255;
    uint32_t* d_obj = reinterpret_cast<uint32_t*>(q); q += (sizeof(uint32_t) * n + 255) & ~(size_t)255;
    DeviceBuildInfo* d_info = reinterpret_cast<DeviceBuildInfo*>(q); q += 256 + ((sizeof(DeviceBuildInfo) + 255) & ~(size_t)255);
    const bool has_obj = ctx->h_obj.size() == n;
    FS_HIP(ctx, hipMemcpyAsync(d_xyz, ctx->h_xyz.data(), sizeof(float) * 9 * n, hipMemcpyHostToDevice, ctx->stream));
    FS_HIP(ctx, hipMemcpyAsync(d_mat, ctx->h_mat.data(), sizeof(uint16_t) * n, hipMemcpyHostToDevice, ctx->stream));
    if (has_obj) FS_HIP(ctx, hipMemcpyAsync(d_obj, ctx->h_obj.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, amax = 0.f;
    for (size_t i = 0; i < 9 * n; ++i) {
        const float v = ctx->h_xyz[i];
        lo[i % 3] = std::min(lo[i % 3], v); hi[i % 3] = std::max(hi[i % 3], v);
        amax = std::max(amax, std::fabs(v));
    }
    const size_t tb = n * sizeof(Tri64);
    if (!reuse) {
        const size_t cap = n + n / 4 + 64;   // room for the next registration
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_nodes, cap * sizeof(NodeQ4)));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_tris, cap * sizeof(Tri64)));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_leaf_pos, sizeof(uint32_t) * cap));
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_node_box, sizeof(float4) * 2 * cap));
        ctx->fast_cap_tris = cap;
    }
    if (!launch_device_build(d_xyz, d_mat, has_obj ? d_obj : nullptr, T, lo, hi, ctx->d_nodes, ctx->d_tris, ctx->d_leaf_pos, q,
                             (size_t)(ctx->d_build + ctx->build_cap - q), d_info, ctx->stream))
        return fs_scene_commit(ctx);
    FS_HIP(ctx, hipGetLastError());
    DeviceBuildInfo info{};
    FS_HIP(ctx, hipMemcpyAsync(&info, d_info, sizeof(info), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info.levels < 1 || info.stack_need > kStackDepth ||
        traversal_lds_bytes(std::min(std::max(info.stack_need, 2) + kStackSlack, ctx->stack_rows_cap + 1), ctx->cfg.num_bands, ctx->num_bins) > ctx->lds_limit)
        return fs_scene_commit(ctx);   // a degenerate Morton tree (deeper than the LDS stack allows): take the host's SAH build
    ctx->bvh = HostBVH{};
    ctx->bvh.nodes.resize((size_t)info.num_nodes); ctx->bvh.tris.resize(n);   // sizes only: the records live on the device
    ctx->bvh.stack_need = info.stack_need;
    ctx->bvh.max_depth = info.levels;
    ctx->bvh.pad = std::max(0.01f, amax * 3.8146973e-06f);                     // as fs_bvh.cpp
    ctx->bvh.level_begin.assign(info.level_begin, info.level_begin + info.levels + 1);
    launch_refit(ctx->d_nodes, ctx->d_tris, ctx->d_node_box, ctx->bvh.level_begin.data(), info.levels, ctx->bvh.pad, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    { int mr = upload_materials(ctx); if (mr) return mr; }
    { const int pr = pack_scene(ctx, n, ctx->fast_cap_tris); if (pr) return pr; }
    return finish_commit(ctx, (size_t)info.num_nodes * sizeof(NodeQ4) + tb + ctx->h_absorption.size() * sizeof(float));
}

// The tree of fs_scene_commit_fast now, the host's SAH tree as soon as it is built (header).
int fs_scene_commit_progressive(fs_context* ctx) {
    const int rc = fs_scene_commit_fast(ctx);
    if (rc) return rc;
    if (ctx->fast_cap_tris == 0) return FS_OK;   // the fast commit took the host's build itself (sharded run, degenerate tree): nothing to refine
    std::shared_ptr<RefineJob> job = std::make_shared<RefineJob>();
    job->xyz = ctx->h_xyz; job->mat = ctx->h_mat;
    if (ctx->h_obj.size() == (size_t)ctx->T) job->obj = ctx->h_obj;
    job->T = ctx->T;
    ctx->refine = job;
    ctx->moved_since_refine = false;
    // a host that re-registers every few frames must not collect thread objects without bound (cancelled builders end
    // within one poll interval)
    if (ctx->refine_threads.size() >= 8) join_refine_threads(ctx);
    ctx->refine_threads.emplace_back([job] {
        build_bvh(job->xyz.data(), job->mat.data(), job->obj.empty() ? nullptr : job->obj.data(), job->T, job->bvh, &job->cancel);
        { std::lock_guard<std::mutex> l(job->mu); job->done = true; }
        job->cv.notify_all();
    });
    return FS_OK;
}

int fs_scene_refine_pending(fs_context* ctx, int32_t* pending) {
    if (!ctx || !pending) return FS_ERR_INVALID_ARGUMENT;
    *pending = ctx->refine ? 1 : 0;
    return FS_OK;
}

int fs_scene_refine_wait(fs_context* ctx) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->refine) return FS_OK;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    wait_refine(ctx->refine);
    return maybe_install_refined(ctx);
}

// ---- moving geometry (row f4): ECC_WorldDynamic movers are seen by the next trace (ARTS.cpp:333-336) -------------
// new_rest: the positions also become the triangles' rest positions (the public call; not the re-apply after a swap)
static int update_triangles(fs_context* ctx, int32_t first, int32_t count, const float* xyz, bool new_rest) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    if (first < 0 || count < 0 || (int64_t)first + count > ctx->T || (count > 0 && !xyz))
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "triangle range outside the committed scene");
    if (count == 0) return FS_OK;
    for (size_t i = 0; i < 9 * (size_t)count; ++i)
        if (!std::isfinite(xyz[i])) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if ((size_t)count > ctx->move_cap) {
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_move) (void)hipFree(ctx->d_move);
        ctx->d_move = nullptr; ctx->move_cap = 0;
        FS_HIP(ctx, hipMalloc((void**)&ctx->d_move, sizeof(float) * 9 * (size_t)count));
        ctx->move_cap = (size_t)count;
    }
    ObjectMoves* mv = new_rest ? ctx->moves : nullptr;
    if (mv) sync_world_positions(ctx);   // an object's pending matrix must not be applied over these positions later
    std::memcpy(ctx->h_xyz.data() + 9 * (size_t)first, xyz, sizeof(float) * 9 * (size_t)count);   // a later commit stays consistent
    if (mv && !mv->rest.empty()) {
        std::memcpy(mv->rest.data() + 9 * (size_t)first, xyz, sizeof(float) * 9 * (size_t)count);
        for (size_t i = 0; i < 9 * (size_t)count; ++i) mv->rest_amax = std::max(mv->rest_amax, (double)std::fabs(xyz[i]));
    }
    if (ctx->refine) ctx->moved_since_refine = true;   // the background tree was built from the old positions
    for (size_t i = 0; i < 9 * (size_t)count; ++i) ctx->amax = std::max(ctx->amax, std::fabs(xyz[i]));
    // the staging buffer may still be read by the previous update's kernel: same stream, so ordered
    FS_HIP(ctx, hipMemcpyAsync(ctx->d_move, xyz, sizeof(float) * 9 * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    launch_update_triangles(ctx->d_tris, ctx->d_tris48, ctx->d_tri_nrm, ctx->d_leaf_pos, first, count, ctx->d_move, view_tris(ctx), ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    if (mv && mv->on_device)   // the device's copy of the rest pose follows
        FS_HIP(ctx, hipMemcpyAsync(mv->d_rest + 9 * (size_t)first, ctx->d_move, sizeof(float) * 9 * (size_t)count, hipMemcpyDeviceToDevice, ctx->stream));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));   // xyz is the caller's memory
    ctx->refit_pending = true;
    ctx->scene_gen += 1;
    return FS_OK;
}

int fs_scene_update_triangles(fs_context* ctx, int32_t first, int32_t count, const float* xyz) {
    return update_triangles(ctx, first, count, xyz, true);
}

// the objects' lists of input indices from h_obj, in order of first appearance (host only)
static void build_object_lists(fs_context* ctx, ObjectMoves* mv) {
    const size_t T = (size_t)ctx->T;
    mv->slot_of.clear();
    std::vector<uint32_t> slot((size_t)T), n;
    for (size_t t = 0; t < T; ++t) {
        const auto it = mv->slot_of.emplace(ctx->h_obj[t], (uint32_t)n.size());
        if (it.second) n.push_back(0);
        slot[t] = it.first->second;
        ++n[slot[t]];
    }
    const size_t slots = n.size();
    mv->off.assign(slots + 1, 0);
    for (size_t k = 0; k < slots; ++k) mv->off[k + 1] = mv->off[k] + n[k];
    mv->idx.resize(T);
    std::vector<uint32_t> at(mv->off.begin(), mv->off.end() - 1);
    for (size_t t = 0; t < T; ++t) mv->idx[at[slot[t]]++] = (uint32_t)t;
    mv->m.assign(12 * slots, 0.f);
    mv->stale.assign(slots, 0);
    mv->seen.assign(slots, 0);
    mv->stale_list.clear();
    mv->stale_list.reserve(slots);
    mv->lists_valid = true;
}

int fs_scene_set_object_transforms(fs_context* ctx, const uint32_t* object_ids, const float* m, int32_t count) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!object_ids || !m || count < 1) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_scene_set_object_transforms: null array or count < 1");
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    FS_FLUSH(ctx);   // pipelined frames: they were traced through the old positions
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    if (ctx->T < 1 || ctx->h_obj.size() != (size_t)ctx->T)
        return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_scene_set_object_transforms: no object ids registered (fs_scene_set_objects)");
    const size_t n = (size_t)count;
    for (size_t i = 0; i < 12 * n; ++i)
        if (!std::isfinite(m[i])) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_scene_set_object_transforms: non-finite matrix entry");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (!ctx->moves) ctx->moves = new ObjectMoves();
    ObjectMoves* mv = ctx->moves;
    if (mv->rest.empty()) {   // the first call since fs_scene_set_triangles: nothing has been transformed yet, h_xyz is the rest pose
        mv->rest = ctx->h_xyz;
        float a = 0.f;
        for (float v : mv->rest) a = std::max(a, std::fabs(v));
        mv->rest_amax = (double)a;
    }
    if (!mv->lists_valid) build_object_lists(ctx, mv);
    // ---- the refusals: nothing has changed up to here but caches
    if (mv->call_slots.size() < n) mv->call_slots.resize(n);
    ++mv->call;
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const auto it = mv->slot_of.find(object_ids[i]);
        if (it == mv->slot_of.end()) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_scene_set_object_transforms: an id owns no committed triangle");
        const uint32_t slot = it->second;
        if (mv->seen[slot] == mv->call) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_scene_set_object_transforms: an id appears twice");
        mv->seen[slot] = mv->call;
        mv->call_slots[i] = slot;
        total += mv->off[slot + 1] - mv->off[slot];
        for (int k = 0; k < 3; ++k) {   // could a transformed coordinate leave fp32?
            const float* r = m + 12 * i + 4 * k;
            const double reach = (std::fabs((double)r[0]) + std::fabs((double)r[1]) + std::fabs((double)r[2])) * mv->rest_amax + std::fabs((double)r[3]);
            if (reach > 3e38) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_scene_set_object_transforms: a transformed coordinate could leave fp32");
        }
    }
    // ---- resources: once per context, per commit, per larger count
    if (!mv->d_amax) {
        FS_HIP(ctx, hipMalloc((void**)&mv->d_amax, sizeof(uint32_t)));
        FS_HIP(ctx, hipMemsetAsync(mv->d_amax, 0, sizeof(uint32_t), ctx->stream));
        FS_HIP(ctx, hipHostMalloc((void**)&mv->h_amax, sizeof(uint32_t), hipHostMallocDefault));
        *mv->h_amax = 0;
        FS_HIP(ctx, hipEventCreateWithFlags(&mv->ev_amax, hipEventDisableTiming));
        for (ObjectMoves::Set& st : mv->set) FS_HIP(ctx, hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    }
    const size_t T = (size_t)ctx->T;
    if (!mv->on_device) {
        if (mv->dev_tris < T) {
            FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (mv->d_rest) (void)hipFree(mv->d_rest);
            if (mv->d_idx) (void)hipFree(mv->d_idx);
            mv->d_rest = nullptr; mv->d_idx = nullptr; mv->dev_tris = 0;
            FS_HIP(ctx, hipMalloc((void**)&mv->d_rest, sizeof(float) * 9 * T));
            FS_HIP(ctx, hipMalloc((void**)&mv->d_idx, sizeof(uint32_t) * T));
            mv->dev_tris = T;
        }
        FS_HIP(ctx, hipMemcpyAsync(mv->d_rest, mv->rest.data(), sizeof(float) * 9 * T, hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(ctx, hipMemcpyAsync(mv->d_idx, mv->idx.data(), sizeof(uint32_t) * T, hipMemcpyHostToDevice, ctx->stream));
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (pageable sources; once per commit)
        mv->on_device = true;
    }
    if (n > mv->cap) {
        FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (ObjectMoves::Set& st : mv->set) {
            if (st.h) (void)hipHostFree(st.h);
            if (st.d) (void)hipFree(st.d);
            st.h = nullptr; st.d = nullptr; st.used = false;
        }
        mv->cap = 0;
        const size_t bytes = sizeof(uint32_t) * (14 * n + 1);
        for (ObjectMoves::Set& st : mv->set) {
            FS_HIP(ctx, hipHostMalloc((void**)&st.h, bytes, hipHostMallocDefault));
            FS_HIP(ctx, hipMalloc((void**)&st.d, bytes));
        }
        mv->cap = n;
    }
    ObjectMoves::Set& st = mv->set[mv->next];
    mv->next = (mv->next + 1) % ObjectMoves::kSets;
    if (st.used && hipEventQuery(st.ev) != hipSuccess) FS_HIP(ctx, hipEventSynchronize(st.ev));   // the call before last has not run yet
    // ---- the call: matrices | prefix | start into the pinned block, one copy, one launch, the 4-byte copy behind it
    float* hm = reinterpret_cast<float*>(st.h);
    uint32_t* hp = reinterpret_cast<uint32_t*>(st.h) + 12 * n;
    uint32_t* hs = hp + (n + 1);
    std::memcpy(hm, m, sizeof(float) * 12 * n);
    hp[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t slot = mv->call_slots[i];
        hp[i + 1] = hp[i] + (mv->off[slot + 1] - mv->off[slot]);
        hs[i] = mv->off[slot];
        std::memcpy(mv->m.data() + 12 * (size_t)slot, m + 12 * i, sizeof(float) * 12);
        if (!mv->stale[slot]) { mv->stale[slot] = 1; mv->stale_list.push_back(slot); }
    }
    if (ctx->refine) ctx->moved_since_refine = true;   // the background tree was built from the old positions
    const size_t bytes = sizeof(uint32_t) * (14 * n + 1);
    FS_HIP(ctx, hipMemcpyAsync(st.d, st.h, bytes, hipMemcpyHostToDevice, ctx->stream));
    const float* dm = reinterpret_cast<const float*>(st.d);
    const uint32_t* dp = reinterpret_cast<const uint32_t*>(st.d) + 12 * n;
    launch_transform_objects(ctx->d_tris, ctx->d_tris48, ctx->d_tri_nrm, ctx->d_leaf_pos, mv->d_rest, mv->d_idx, dp, dp + (n + 1), dm,
                             (int)n, (uint32_t)total, mv->d_amax, view_tris(ctx), ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    FS_HIP(ctx, hipEventRecord(st.ev, ctx->stream));
    st.used = true;
    FS_HIP(ctx, hipMemcpyAsync(mv->h_amax, mv->d_amax, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    FS_HIP(ctx, hipEventRecord(mv->ev_amax, ctx->stream));
    mv->amax_pending = true;
    ctx->refit_pending = true;
    ctx->scene_gen += 1;
    return FS_OK;
}

int fs_scene_refit(fs_context* ctx) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    ctx->refit_pending = false;
    if (ctx->bvh.nodes.empty()) { ctx->scene_gen += 1; return FS_OK; }
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    FS_HIP(ctx, fold_moved_amax(ctx));   // objects moved by transform: the device knows how far
    const float pad = std::max(std::max(0.01f, ctx->amax * 3.8146973e-06f), ctx->bvh.pad);   // as fs_bvh.cpp; never shrinks
    launch_refit(ctx->d_nodes, ctx->d_tris, ctx->d_node_box, ctx->bvh.level_begin.data(),
                 (int)ctx->bvh.level_begin.size() - 1, pad, ctx->stream);
    FS_HIP(ctx, hipGetLastError());
    { const int cr = refresh_coop_nodes(ctx, false); if (cr) return cr; }
    { const int vr = refresh_node_view(ctx, false); if (vr) return vr; }
    ctx->scene_gen += 1;
    return FS_OK;
}

// Debug entry (not in include/frequensee.h; tests/tree_check.py reads the committed tree through it): one array of the
// committed scene copied to host memory, sized for the scene — not for the capacity a fast commit keeps.  Read-only: held
// frames are flushed and the compute stream drains as in the other scene calls, but a pending refit stays pending and
// nothing is launched.  what: 0 header {nodes, triangles, levels, stack_need, bvh.pad, amax, coop16_nodes, coop_levels,
// refit_pending, arrays of a fast commit, 0, 0} (12 x 4 B) | 1 NodeQ4[nodes] | 2 Tri64[T] | 3 Tri48[T] | 4 normals[T] |
// 5 leaf_pos[T] | 6 level_begin[levels + 1] (host copy) | 7 CoopChild[4 nodes] | 8 CoopChild[16 coop16_nodes] |
// 9 d_coop_levels [2][kMaxBuildLevels + 2] | 10 node_box[nodes][2] | 11 ViewRec[nodes + T] (the 48-byte node view; no bytes
// if the scene has none) | 12 its normals[nodes + T] | 13 leaf order -> view record [T].  cap too small: FS_ERR_SIZE_MISMATCH,
// *bytes = the size.
__attribute__((visibility("default"))) int fs_debug_scene_snapshot(fs_context* ctx, int32_t what, void* out, size_t cap, size_t* bytes) {
    if (!ctx || !bytes) return FS_ERR_INVALID_ARGUMENT;
    *bytes = 0;
    if (!ctx->device_ok) return ctx->fail(FS_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    if (!ctx->committed) return ctx->fail(FS_ERR_NOT_COMMITTED, "scene not committed");
    FS_HIP(ctx, hipSetDevice(ctx->cfg.device));
    FS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FS_HIP(ctx, fold_moved_amax(ctx));
    const size_t nodes = ctx->bvh.nodes.size(), T = (size_t)ctx->T;
    const size_t levels = ctx->bvh.level_begin.empty() ? 0 : ctx->bvh.level_begin.size() - 1;
    uint32_t hdr[12] = {(uint32_t)nodes, (uint32_t)T, (uint32_t)levels, (uint32_t)ctx->bvh.stack_need, 0, 0,
                        (uint32_t)ctx->coop16_nodes, (uint32_t)ctx->coop_levels, ctx->refit_pending ? 1u : 0u,
                        ctx->fast_cap_tris > 0 ? 1u : 0u, 0, 0};
    std::memcpy(&hdr[4], &ctx->bvh.pad, sizeof(float));
    std::memcpy(&hdr[5], &ctx->amax, sizeof(float));
    const void* src = nullptr;
    bool on_device = true;
    size_t need = 0;
    switch (what) {
        case 0: src = hdr; need = sizeof(hdr); on_device = false; break;
        case 1: src = ctx->d_nodes; need = nodes * sizeof(NodeQ4); break;
        case 2: src = ctx->d_tris; need = T * sizeof(Tri64); break;
        case 3: src = ctx->d_tris48; need = T * sizeof(Tri48); break;
        case 4: src = ctx->d_tri_nrm; need = T * sizeof(float4); break;
        case 5: src = ctx->d_leaf_pos; need = T * sizeof(uint32_t); break;
        case 6: src = ctx->bvh.level_begin.data(); need = ctx->bvh.level_begin.size() * sizeof(int32_t); on_device = false; break;
        case 7: src = ctx->d_coop; need = 4 * nodes * sizeof(CoopChild); break;
        case 8: src = ctx->d_coop16; need = 16 * (size_t)ctx->coop16_nodes * sizeof(CoopChild); break;
        case 9: src = ctx->d_coop_levels; need = ctx->d_coop_levels ? 2 * (size_t)(kMaxBuildLevels + 2) * sizeof(int32_t) : 0; break;
        case 10: src = ctx->d_node_box; need = 2 * nodes * sizeof(float4); break;
        case 11: src = ctx->d_view; need = ctx->view_ok ? (nodes + T) * sizeof(ViewRec) : 0; break;
        case 12: src = ctx->d_view_nrm; need = ctx->view_ok ? (nodes + T) * sizeof(float4) : 0; break;
        case 13: src = ctx->d_view_of_leaf; need = ctx->view_ok ? T * sizeof(uint32_t) : 0; break;
        default: return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_debug_scene_snapshot: no such array");
    }
    *bytes = need;
    if (need == 0) return FS_OK;
    if (!src) return ctx->fail(FS_ERR_INVALID_ARGUMENT, "fs_debug_scene_snapshot: the scene holds no such array");
    if (!out || cap < need) return ctx->fail(FS_ERR_SIZE_MISMATCH, "fs_debug_scene_snapshot: buffer too small");
    if (on_device) FS_HIP(ctx, hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    else std::memcpy(out, src, need);
    return FS_OK;
}

// Debug entry (not in include/frequensee.h): on = 0 — the committed scene loses its 48-byte node view and later commits build
// none, so that fused frames take the route of a scene that cannot have one (launch_frame, fs_frame.hip); on = 1 — commits
// build it again (the scene in place gets it back with its next commit).
__attribute__((visibility("default"))) int fs_debug_set_node_view(fs_context* ctx, int32_t on) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    FS_FLUSH(ctx);   // pipelined frames: a held-back connect pass goes first
    ctx->view_off = on == 0;
    if (ctx->view_off) { ctx->view_ok = false; ctx->coop_info.view = NodeView{}; }
    return FS_OK;
}

// Debug entry: the view's size rule (fs_internal.hpp: node_view_fits), for the tests of its boundary.  Host arithmetic only.
__attribute__((visibility("default"))) int fs_debug_node_view_fits(uint64_t nodes, uint64_t triangles) {
    return node_view_fits(nodes, triangles) ? 1 : 0;
}
static_assert(node_view_fits(1, 0xFFFFFFFFull / sizeof(ViewRec) - 1) && !node_view_fits(1, 0xFFFFFFFFull / sizeof(ViewRec)),
              "the last record's byte offset must fit 32 bits");

int fs_scene_set_objects(fs_context* ctx, const uint32_t* object_id, int32_t T) {
    if (!ctx) return FS_ERR_INVALID_ARGUMENT;
    if (object_id && T != ctx->T) return ctx->fail(FS_ERR_SIZE_MISMATCH, "object ids: T != number of triangles");
    if (object_id) ctx->h_obj.assign(object_id, object_id + T);
    else ctx->h_obj.clear();
    ctx->committed = false;
    return FS_OK;
}

}  // extern "C"
