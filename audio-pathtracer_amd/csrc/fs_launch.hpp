// fs_launch.hpp — host-side helpers of the kernel launchers: LDS sizes and limits, the deep store, the passes' grid rules, the
// cooperative traversal's node arrays.
#pragma once

#include "fs_dev_coop.hpp"   // (the cooperative kernels' LDS layout: kCoopCap, kCoopWaveBytes)

namespace fs {
namespace {

// dynamic LDS of a traversal kernel: the scene's stack rows (+ extra bytes behind them).  Sizes above the default
// 48 KB limit are announced to the runtime once per (kernel instantiation, device); the host side has already
// checked the worst case against the device's LDS (fs_capi.cpp: lds_budget_ok), so a failure here is unexpected
// and is left for the launch's own error to report.
#ifdef FS_EXPERIMENTS
#define FS_SHARED_WALK(wl) ((wl).variant == 2)
#else
#define FS_SHARED_WALK(wl) true
#endif
inline size_t stack_bytes(const DeviceScene& sc) { return sizeof(int) * (size_t)sc.stack_rows * (size_t)kBlock; }
// The deep store must have a column for every lane of the grid about to be launched (DeviceScene.deep).  Grows it if
// not — a new buffer; the old one stays allocated for the launches already in the stream (DeepStore.retired).
// false: the allocation failed, the launch must be skipped (DeepStore.failed is set; the host reports it).
inline bool attach_deep(DeviceScene& sc, uint32_t blocks) {
    DeepStore* d = sc.deep_owner;
    if (d == nullptr || d->rows <= 0) { sc.deep = nullptr; sc.deep_lanes = 0; return true; }
    const size_t lanes = (size_t)blocks * kBlock;
    if (lanes > d->lanes) {
        size_t want = std::max<size_t>(d->lanes * 2, 2048 * (size_t)kBlock);
        while (want < lanes) want *= 2;
        int32_t* nb = nullptr;
        if (hipMalloc((void**)&nb, sizeof(int32_t) * want * (size_t)d->rows) != hipSuccess) { (void)hipGetLastError(); d->failed = true; return false; }
        if (d->buf) d->retired.push_back(d->buf);
        d->buf = nb; d->lanes = want;
    }
    sc.deep = d->buf; sc.deep_lanes = (uint32_t)d->lanes;
    return true;
}
// ---- one grid rule per pass: the stand-alone launchers and the fused one (fs_frame.hip) ask here; each keeps its own cap ----
// workgroups the connect pass wants: a wave steps through pairs_per_wave pairs at a time; the sources of a batched frame
// (per-source buffers) each start on workgroups of their own
inline uint32_t connect_blocks_wanted(uint32_t num_local, uint32_t pairs_per_source, int pairs_per_wave, bool batch) {
    const uint32_t per_block = (uint32_t)pairs_per_wave * (kBlock / 64);
    return batch ? (num_local / pairs_per_source) * ((pairs_per_source + per_block - 1) / per_block) : (num_local + per_block - 1) / per_block;
}
// lanes of a walk part — a later stage only has lanes for the walks still alive (its slots_cap is filled in here) — and the
// workgroups of four waves that walk them on sparse (rays_per_wave < 64: the other lanes help) or dense (64) waves
inline uint32_t walk_part_lanes(const KParams& kp, WalkStage& stage) {
    if (stage.begin > 0 && stage.slots_cap == 0xFFFFFFFFu) stage.slots_cap = walk_stage_slots(kp, stage.begin);
    return stage.begin > 0 ? stage.slots_cap : 2u * kp.num_local;
}
inline uint32_t walk_blocks(uint32_t lanes, int rays_per_wave) {
    const uint32_t waves = (lanes + (uint32_t)rays_per_wave - 1) / (uint32_t)rays_per_wave;
    return (waves + kBlock / 64 - 1) / (kBlock / 64);
}
constexpr int kMaxDevices = 64;
// LDS one workgroup may have on the current device (MI355X: all 160 KB of its CU)
inline size_t device_lds_per_block() {
    static std::atomic<int> cached[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) v = 64 * 1024;
        cached[dev].store(v, std::memory_order_relaxed);
    }
    return (size_t)v;
}
// How many nodes of the breadth-first array a cooperative kernel stages in every workgroup's LDS: all of the tree if it
// fits, else its top.  A launch whose workgroups all fit the chip at once (one per CU) may take the CU's whole LDS; one
// that comes in rounds leaves room for a second workgroup per CU.
inline int coop_resident_nodes(const CoopView& cv, int waves_per_block, uint32_t blocks, int num_cus) {
    // (three workgroups of four waves per CU instead of one of eight, or LDS sized for three: 0.624 / 0.603 / 0.603 ms per 32-source tick — no setting)
    const size_t cu_lds = 160 * 1024, per_block = std::min(device_lds_per_block(), blocks <= (uint32_t)std::max(num_cus, 1) ? cu_lds : cu_lds / 2);
    const size_t fixed = kCoopWaveBytes * (size_t)waves_per_block + 1024;   // + the kernels' small static arrays
    if (per_block <= fixed || !cv.rec) return 0;
    return (int)std::min<size_t>((size_t)std::max(cv.nodes, 0), (per_block - fixed) / ((size_t)16 << cv.wshift));
}
template <typename K>
inline void allow_lds(K kernel, size_t bytes) {
    static std::atomic<size_t> allowed[kMaxDevices];   // per kernel instantiation; 0 = the default limit
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    const size_t have = std::max<size_t>(allowed[dev].load(std::memory_order_relaxed), 48 * 1024);
    if (bytes > have &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess)
        allowed[dev].store(bytes, std::memory_order_relaxed);
}

// may R rays share a wave on this tree?  (a group's share of the node stack must hold the worst-case descent + one wide step)
inline bool coop_fits(const CoopView& cv, int R) {
    const int per = (1 << cv.wshift) - 1, kfull = std::max(1, (64 / R) >> cv.wshift);
    return cv.rec != nullptr && cv.nodes > 0 && (64 / R) >= (1 << cv.wshift) && cv.stack_need + 8 + per * kfull <= kCoopCap / R;
}
// the node array waves of R rays walk: 16-wide nodes for 1 and 2 rays per wave, 4-wide for 4 (the other one if it does not fit)
inline const CoopView* coop_view(const DeviceScene& sc, int R) {
    if (!sc.coop_info) return nullptr;
    const CoopView* v = (R == 1 || R == 2) ? &sc.coop_info->wide16 : &sc.coop_info->wide4;
    if (!coop_fits(*v, R)) v = v == &sc.coop_info->wide16 ? &sc.coop_info->wide4 : &sc.coop_info->wide16;
    return coop_fits(*v, R) ? v : nullptr;
}
// dynamic LDS of a cooperative kernel launched with `waves` waves per workgroup and the view's resident nodes
inline size_t coop_lds_bytes(int waves, const CoopView& cv) { return ((size_t)cv.lds_nodes << cv.wshift) * 16u + kCoopWaveBytes * (size_t)waves; }

}  // namespace
}  // namespace fs
