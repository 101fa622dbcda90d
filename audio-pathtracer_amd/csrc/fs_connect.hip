// fs_connect.hip — ConnectSubpaths + EvaluatePath + deposit kernels (AudioRayTracingSubsystem.cpp:235-277, 360-420;
// FrequenSeeAudioComponent.h:87-91), the all-prefix variant (draft :518-546, row f3) and the fixed-point rounding pass.
#include "fs_dev_connect.hpp"
#include "fs_launch.hpp"

namespace fs {
namespace {

template <int B, int LOBES, bool BATCH, bool COUNT, bool EXT = false, int AHEAD = 1>
__global__ __launch_bounds__(kBlock, AHEAD > 4 ? 2 : 4) void connect_kernel(DeviceScene sc, KParams kp, SubpathState st,
                                                         float* __restrict__ energy,
                                                         unsigned long long* __restrict__ fixed, unsigned* queue_head,
                                                         int pairs_per_wave, float* const* __restrict__ energy_tab,
                                                         unsigned long long* const* __restrict__ fixed_tab) {
    connect_body<B, LOBES, BATCH, COUNT, EXT, AHEAD>(blockIdx.x, gridDim.x, sc, kp, st, energy, fixed, queue_head, pairs_per_wave, energy_tab, fixed_tab);
}
// a directional source (fs_source_set_directivity): the same pass, every deposit weighted by D_b(w_e) — an entry of its own, so
// that the kernels above keep their arguments
template <int B, int LOBES, bool BATCH, bool COUNT, bool EXT = false, int AHEAD = 1>
__global__ __launch_bounds__(kBlock, AHEAD > 4 ? 2 : 4) void connect_dir_kernel(DeviceScene sc, KParams kp, SubpathState st,
                                                             float* __restrict__ energy,
                                                             unsigned long long* __restrict__ fixed, unsigned* queue_head,
                                                             int pairs_per_wave, float* const* __restrict__ energy_tab,
                                                             unsigned long long* const* __restrict__ fixed_tab, DirArgs dir) {
    connect_body<B, LOBES, BATCH, COUNT, EXT, AHEAD, true>(blockIdx.x, gridDim.x, sc, kp, st, energy, fixed, queue_head, pairs_per_wave,
                                                          energy_tab, fixed_tab, dir);
}

// ---------------------------------------------------------------------------------------------------
// connect_all_kernel (row f3): the reference's unfinished "naive connections" (Is_NaiveConnections,
// ARTS.cpp:518-546: every bounce of the forward sample x every bounce of the backward sample, "Equation 12").
// For pair p with forward nodes F0..Fk and backward nodes B0..Bm every (i, j) in [0,k] x [0,m] is a
// candidate path F0..Fi, Bj..B0: ConnectSubpaths' visibility test Fi -> Bj, EvaluatePath over the stored
// segment records in path order, uniform multiple-importance weight 1 / N(i + j) with N(t) = number of
// (i', j') in [0, D]^2, i' + j' = t (D = depth cap).  One WAVE per pair, one lane per (i, j): the up to
// (D+1)^2 visibility rays of a pair start and end at neighbouring nodes, so the wave traverses coherently.
// ---------------------------------------------------------------------------------------------------
// Balance-heuristic weight of strategy i (vertices y_1..y_i generated from the source, y_t..y_{i+1} from the
// listener, t = i + j) among the strategies [max(0, t-D), min(t, D)] that give the same path — the intent of the
// draft's MISEnergy (ARTS.cpp:571-597); build-owned definition, DESIGN.md section 8: forward density of y_{k+1}
// given y_k  pf_k = Pf(k) |n_{k+1}.d_k| / L_k^2 with Pf(0) = 1/4pi, Pf(k) = max(0, n_k.d_k)/pi; backward density of
// y_k given y_{k+1}  pb_k = Pb(k+1) |n_k.d_k| / L_k^2 with Pb(t+1) = 1/4pi, Pb(k) = max(0, -n_k.d_{k-1})/pi;
// p_s = prod_{k<s} pf_k prod_{k>s} pb_k, w_i = p_i / sum_s p_s.  One pass over the t + 1 segments in double:
// T_k = T_{k-1} pb_k + [lo <= k <= hi] PF_k ends as sum_s p_s, Q likewise as p_i; uniform weight when a segment
// is degenerate or the ratio is not finite and positive.
// Vertex k of the connected path: 0 = source, 1..i = forward nodes, i+1..t = backward nodes j..1, t+1 = listener.
struct MisVertex { double x, y, z, nx, ny, nz; };
__device__ __forceinline__ MisVertex mis_vertex(const KParams& kp, const SubpathState& st, uint32_t total, uint32_t sf,
                                                uint32_t sl, int i, int t, int k) {
    MisVertex v;
    if (k == 0) { v.x = kp.src[0]; v.y = kp.src[1]; v.z = kp.src[2]; v.nx = v.ny = v.nz = 0.0; return v; }
    if (k == t + 1) { v.x = kp.lis[0]; v.y = kp.lis[1]; v.z = kp.lis[2]; v.nx = v.ny = v.nz = 0.0; return v; }
    const float4 q = k <= i ? load_pos(st, total, k - 1, sf) : load_pos(st, total, t - k, sl);
    const float4 m = k <= i ? load_nrm(st, total, k - 1, sf) : load_nrm(st, total, t - k, sl);
    v.x = q.x; v.y = q.y; v.z = q.z; v.nx = m.x; v.ny = m.y; v.nz = m.z;
    return v;
}
__device__ float mis_weight(const KParams& kp, const SubpathState& st, uint32_t total, uint32_t sf, uint32_t sl, int i,
                            int j) {
    const int t = i + j, D = kp.mis_depth;
    const int lo = t - D > 0 ? t - D : 0, hi = t < D ? t : D;
    const double uniform = 1.0 / (double)(hi - lo + 1);
    if (t <= 0) return (float)uniform;
    const double inv4pi = 1.0 / (4.0 * 3.14159265358979323846), invpi = 1.0 / 3.14159265358979323846;
    double PF = 1.0, T = 0.0, Q = 0.0;
    MisVertex a = mis_vertex(kp, st, total, sf, sl, i, t, 0);
    for (int k = 0; k <= t; ++k) {
        const MisVertex b = mis_vertex(kp, st, total, sf, sl, i, t, k + 1);
        double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
        const double l2 = dx * dx + dy * dy + dz * dz;
        if (!(l2 > 1e-8)) return (float)uniform;
        const double inv = 1.0 / sqrt(l2);
        dx *= inv; dy *= inv; dz *= inv;
        const double ca = k > 0 ? a.nx * dx + a.ny * dy + a.nz * dz : 0.0;
        const double cb = k < t ? b.nx * dx + b.ny * dy + b.nz * dz : 0.0;
        if (k >= 1) {
            const double Pb = k == t ? inv4pi : (cb < 0.0 ? -cb : 0.0) * invpi;
            const double pb = Pb * fabs(ca) / l2;
            T *= pb;
            if (k > i) Q *= pb;
        }
        if (k >= lo && k <= hi) T += PF;
        if (k == i) Q = PF;
        if (k < t) {
            const double Pf = k == 0 ? inv4pi : (ca > 0.0 ? ca : 0.0) * invpi;
            PF *= Pf * fabs(cb) / l2;
        }
        a = b;
    }
    const double w = Q / T;
    if (!(Q > 0.0) || !(T > 0.0) || !(w <= 1.0)) return (float)uniform;
    return (float)w;
}

#define FS_CONNECT_ALL_DIR 0
#include "fs_connect_all.inc"
#undef FS_CONNECT_ALL_DIR
#define FS_CONNECT_ALL_DIR 1
#include "fs_connect_all.inc"
#undef FS_CONNECT_ALL_DIR

// deterministic mode: fixed-point histogram -> the fp32 energy buffer (one rounding per bin, after all sums)
__global__ __launch_bounds__(kBlock) void fixed_to_energy_kernel(const unsigned long long* __restrict__ fixed,
                                                                 float* __restrict__ energy, int words) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < words) energy[i] = (float)((double)fixed[i] * (1.0 / kFixedScale));
}

// segment records a lane requests at once when it evaluates an uncapped walk's path alone (connect_body's AHEAD; eight in
// flight measured too: DESIGN.md section 8, profiles/r05_connect_records_ahead.jsonl)
constexpr int kConnectAhead = 4;

template <int B>
void launch_connect_t(const DeviceScene& sc_in, const ConnectPass& c, hipStream_t s, const DirArgs* dir) {
    // (the kernels' arguments, in their order)
    const KParams& kp = c.kp;
    const SubpathState& st = c.st;
    float* const energy = c.energy; unsigned long long* const fixed = c.fixed; unsigned* const queue_head = c.scratch;
    float* const* const energy_tab = c.energy_tab; unsigned long long* const* const fixed_tab = c.fixed_tab;
    if (kp.num_local == 0) return;
    DeviceScene sc = sc_in;
    const int pairs_per_wave = c.pairs_per_wave < 1 || c.pairs_per_wave > 64 ? 64 : c.pairs_per_wave;
    const bool batch = energy_tab != nullptr;
    const uint32_t blocks = std::min<uint32_t>(connect_blocks_wanted(kp.num_local, kp.pairs_per_source, pairs_per_wave, batch), 1024u);
    if (!attach_deep(sc, blocks)) return;
    size_t lds = stack_bytes(sc) + sizeof(float) * (size_t)kp.num_bands * (size_t)kp.hist_window + kShareAnyLdsBytes;
#define FS_LAUNCH_CONNECT(L, BT, CN)                                                                                 \
    do {                                                                                                             \
        allow_lds(connect_kernel<B, L, BT, CN>, lds);                                                                \
        hipLaunchKernelGGL((connect_kernel<B, L, BT, CN>), dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, energy,   \
                           fixed, queue_head, pairs_per_wave, energy_tab, fixed_tab);                                \
    } while (0)
    // a directional source: the EXT pass's shape (run-time band count and lobes) through the directional entry
    if (dir) {
        if (B != 0) return launch_connect_t<0>(sc, c, s, dir);
        if (batch) {
            allow_lds(connect_dir_kernel<0, -1, true, false, true>, lds);
            hipLaunchKernelGGL((connect_dir_kernel<0, -1, true, false, true>), dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, energy, fixed,
                               queue_head, pairs_per_wave, energy_tab, fixed_tab, *dir);
        } else {
            allow_lds(connect_dir_kernel<0, -1, false, false, true>, lds);
            hipLaunchKernelGGL((connect_dir_kernel<0, -1, false, false, true>), dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, energy, fixed,
                               queue_head, pairs_per_wave, energy_tab, fixed_tab, *dir);
        }
        return;
    }
    // FS_FLAG_DOUBLE_POSITIONS / end-point collision spheres: one instantiation pair with the run-time band count and run-time lobes
    if (kp.dpos || kp.listener_radius > 0.0f || kp.source_radius > 0.0f) {
        if (B != 0) return launch_connect_t<0>(sc, c, s, dir);
        if (batch) {
            allow_lds(connect_kernel<0, -1, true, false, true>, lds);
            hipLaunchKernelGGL((connect_kernel<0, -1, true, false, true>), dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, energy, fixed,
                               queue_head, pairs_per_wave, energy_tab, fixed_tab);
        } else {
            allow_lds(connect_kernel<0, -1, false, false, true>, lds);
            hipLaunchKernelGGL((connect_kernel<0, -1, false, false, true>), dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, energy, fixed,
                               queue_head, pairs_per_wave, energy_tab, fixed_tab);
        }
        return;
    }
    // uncapped walks (the waited-for frames; the pipelined ones connect inside the fused launch): paths of up to a few hundred
    // segments, evaluated by ONE lane when the wave is dense — kConnectAhead records in flight (connect_body's AHEAD)
    if (st.over_levels != 0 && !kp.lobes && !kp.count) {
        if (batch) {
            allow_lds(connect_kernel<B, 0, true, false, false, kConnectAhead>, lds);
            hipLaunchKernelGGL((connect_kernel<B, 0, true, false, false, kConnectAhead>), dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, energy, fixed, queue_head,
                               pairs_per_wave, energy_tab, fixed_tab);
        } else {
            allow_lds(connect_kernel<B, 0, false, false, false, kConnectAhead>, lds);
            hipLaunchKernelGGL((connect_kernel<B, 0, false, false, false, kConnectAhead>), dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, energy, fixed, queue_head,
                               pairs_per_wave, energy_tab, fixed_tab);
        }
        return;
    }
    // record-fetch counting (fs_set_profiling level 3) exists for the default frame shape only
    if (batch) { if (kp.lobes) FS_LAUNCH_CONNECT(1, true, false); else FS_LAUNCH_CONNECT(0, true, false); }
    else if (kp.lobes) FS_LAUNCH_CONNECT(1, false, false);
    else if (kp.count) FS_LAUNCH_CONNECT(0, false, true);
    else FS_LAUNCH_CONNECT(0, false, false);
#undef FS_LAUNCH_CONNECT
}

template <int B>
void launch_connect_all_t(const DeviceScene& sc_in, const ConnectPass& c, hipStream_t s, const DirArgs* dir) {
    const KParams& kp = c.kp;
    const SubpathState& st = c.st;
    if (kp.num_local == 0) return;
    DeviceScene sc = sc_in;
    uint32_t blocks = (kp.num_local + 3) / 4;   // one wave per pair, 4 waves per workgroup
    if (blocks > 4096) blocks = 4096;
    if (!attach_deep(sc, blocks)) return;
    size_t lds = stack_bytes(sc) + sizeof(float) * (size_t)kp.num_bands * (size_t)kp.hist_window + kShareAnyLdsBytes;
    if (dir) {
        allow_lds(connect_all_dir_kernel<B>, lds);
        hipLaunchKernelGGL(connect_all_dir_kernel<B>, dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, c.energy, c.fixed, c.scratch, *dir);
        return;
    }
    allow_lds(connect_all_kernel<B>, lds);
    hipLaunchKernelGGL(connect_all_kernel<B>, dim3(blocks), dim3(kBlock), lds, s, sc, kp, st, c.energy, c.fixed, c.scratch);
}

}  // namespace

void launch_connect(int B, const DeviceScene& sc, const ConnectPass& c, hipStream_t s, const DirArgs* dir) {
    // instantiated for the band counts in use (the reference: 1; BASELINE.json's configurations: 4 and 8); B = 0 reads
    // kp.num_bands at run time
    switch (B) {
        case 1: launch_connect_t<1>(sc, c, s, dir); break;
        case 4: launch_connect_t<4>(sc, c, s, dir); break;
        case 8: launch_connect_t<8>(sc, c, s, dir); break;
        default: launch_connect_t<0>(sc, c, s, dir); break;
    }
}

void launch_connect_all(int B, const DeviceScene& sc, const ConnectPass& c, hipStream_t s, const DirArgs* dir) {
    switch (B) {
        case 1: launch_connect_all_t<1>(sc, c, s, dir); break;
        case 4: launch_connect_all_t<4>(sc, c, s, dir); break;
        case 8: launch_connect_all_t<8>(sc, c, s, dir); break;
        default: launch_connect_all_t<0>(sc, c, s, dir); break;
    }
}

void launch_fixed_to_energy(const unsigned long long* fixed, float* energy, int words, hipStream_t s) {
    if (words <= 0) return;
    hipLaunchKernelGGL(fixed_to_energy_kernel, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, fixed,
                       energy, words);
}

}  // namespace fs
