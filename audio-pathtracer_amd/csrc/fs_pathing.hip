// fs_pathing.hip — fs_pathing_bake and fs_update_pathing_paths: the probe graph that carries a source's sound round several corners.
// The definitions (candidate pairs, edges, the listener's attach distances, the fixed point d, pred, the per-source rule) are those
// of include/frequensee.h "pathing", operation by operation; this file is their mapping onto the device.  Every visibility test is
// chain(o, d, len) with max_surfaces = 0: path_chain<StopAtHit> of fs_dev_paths.hpp.
//   pathing_bake_kernel: one wave per (row i, block of 64 columns j), four tasks per workgroup; only the blocks on and right of the
// diagonal's are launched, enumerated row block by row block.  Lanes with j > i that are candidates run the chain p_i -> p_j, the
// others idle along in the wave-uniform loop; a ballot gives the 64-bit piece of the row, stored by lanes 0 and 1 as two words of
// `upper`.  No atomics.
//   pathing_mirror_kernel: one thread per word of `graph`: the bits right of the diagonal from `upper`'s own row, the bits left of
// it from the rows above (bit i of row j).  It reads `upper` and writes `graph` only: no word is read and written in one launch.
//   pathing_attach_kernel: the listener's attach chains, a thread per probe; dL goes to memory.
//   pathing_relax_kernel: ONE workgroup of 1024 threads, a probe per thread and no traversal stack.  Jacobi rounds of the relaxation
// with the probes' positions, dL and d (two arrays, read one, write the other: 24 KB) in LDS and the adjacency rows read from memory
// (L2), a whole row in flight at once, until a workgroup-wide "nothing changed", under a hard cap of n rounds written into the loop;
// then pred.  d and pred go to memory for the sources' kernel.  (Sixteen waves and not four: a neighbour visit is three LDS reads
// and a correctly rounded sqrtf one after the other, and a SIMD with one wave has nothing else to issue meanwhile.)
//   pathing_sources_kernel: one workgroup per source row.  The threads stride over the probes (and one more index, the DIRECT ray)
// with their attach chains; the minimum over the key (total's bits, k) is a tree over LDS in a fixed order; thread 0 walks pred
// into LDS; wave 0 fills the row and runs the validation legs 64 at a time.
//   Dynamic LDS of the kernels that run chains: the stack rows [stack_rows][kBlock], then the sources' kernel's own arrays (kSourcesLds).
#include "fs_dev_paths.hpp"

namespace fs {
namespace {

constexpr int kMaxProbes = FS_MAX_PATHING_PROBES;
constexpr uint32_t kListener = 0xFFFFFFFFu;   // pred of a probe the listener attaches to
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kRelaxBlock = 1024;             // the relaxation's one workgroup: sixteen waves, a probe per thread
constexpr size_t kSourcesLds = sizeof(unsigned long long) * (size_t)kBlock + sizeof(uint32_t) * ((size_t)kMaxProbes + 4);   // keys | path | flag, hops
constexpr int kRowWords = (int)(sizeof(fs_pathing_path) / sizeof(uint32_t));
static_assert(sizeof(fs_pathing_path) == 152 && kRowWords <= 64, "a row is written by one wave, a word per lane where it is zeroed");

// e = b - a per component, w = sqrtf(e.e), d = e (1.0f / w): the bake's pair, an attach leg, the DIRECT ray
struct Leg {
    float dx, dy, dz, w;
};
__device__ __forceinline__ Leg leg_between(float ax, float ay, float az, float bx, float by, float bz) {
    Leg l;
    const float ex = bx - ax, ey = by - ay, ez = bz - az;
    l.w = sqrtf((ex * ex + ey * ey) + ez * ez);
    const float inv = 1.0f / l.w;
    l.dx = ex * inv; l.dy = ey * inv; l.dz = ez * inv;
    return l;
}

// the own actors of a baked leg: none
__device__ __forceinline__ PathKHead no_actors(PathKHead h) {
    h.lis_object = FS_NO_OBJECT;
    return h;
}

__global__ __launch_bounds__(kBlock) void pathing_bake_kernel(DeviceScene sc, PathingBakeKParams bp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock]
    int* stack = &s_dyn[threadIdx.x];
    const int lane = (int)(threadIdx.x & 63u);
    const int n = bp.g.n, nb = (n + 63) >> 6;
    // the wave's task -> (row i, column block jb): row block ib has min(64, n - 64 ib) rows of nb - ib blocks each
    int t = (int)(blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6)), i = -1, jb = 0;
    for (int ib = 0; ib < nb; ++ib) {
        const int per = nb - ib, tasks = min(64, n - ib * 64) * per;
        if (t < tasks) { i = ib * 64 + t / per; jb = ib + t % per; break; }
        t -= tasks;
    }
    const bool task_ok = i >= 0;   // (a wave beyond the last task idles along)
    const int j = jb * 64 + lane;
    const float4 pi = bp.g.probes[task_ok ? i : 0];
    const float4 pj = bp.g.probes[min(j, n - 1)];
    const Leg l = leg_between(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z);
    const bool candidate = task_ok && j > i && j < n && l.w >= FS_PATHING_MIN_EDGE && l.w <= bp.max_edge;
    const int end = path_chain(sc, bp.h, FS_NO_OBJECT, candidate, pi.x, pi.y, pi.z, l.dx, l.dy, l.dz, l.w, stack, StopAtHit{});
    const unsigned long long piece = __ballot(candidate && end == kChainReached);
    if (task_ok && lane < 2) bp.g.upper[(size_t)i * bp.g.stride + 2 * jb + lane] = (uint32_t)(piece >> (32 * lane));
}

__global__ __launch_bounds__(kBlock) void pathing_mirror_kernel(PathingSet g) {
    const int idx = (int)(blockIdx.x * kBlock + threadIdx.x);
    const int i = idx / g.stride, w = idx % g.stride;
    if (i >= g.n) return;
    uint32_t word = w >= 2 * (i >> 6) ? g.upper[(size_t)i * g.stride + w] : 0u;   // (a piece holds no bit j <= i)
    for (int b = 0; b < 32; ++b) {
        const int j = 32 * w + b;
        if (j < i) word |= ((g.upper[(size_t)j * g.stride + (i >> 5)] >> (i & 31)) & 1u) << b;
    }
    g.graph[idx] = word;
}

// visit(j) for every neighbour j of probe i, ascending.  The row's words are all requested before the first is looked at: one
// wait for memory per probe, not one per word (read one after the other, a row at 1024 probes is 32 dependent loads).
template <typename Visit>
__device__ __forceinline__ void for_each_neighbour(const PathingSet& g, int i, Visit&& visit) {
    const uint32_t* row = g.graph + (size_t)i * g.stride;
    uint32_t words[kPathingStrideWords];
#pragma unroll
    for (int w = 0; w < kPathingStrideWords; ++w) words[w] = w < g.stride ? row[w] : 0u;
#pragma unroll
    for (int w = 0; w < kPathingStrideWords; ++w) {
        uint32_t word = words[w];
        while (word != 0u) {
            const int j = 32 * w + (__ffs((int)word) - 1);
            word &= word - 1u;
            visit(j);
        }
    }
}

__global__ __launch_bounds__(kBlock) void pathing_attach_kernel(DeviceScene sc, PathingKParams pp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock]
    int* stack = &s_dyn[threadIdx.x];
    const int k = (int)(blockIdx.x * kBlock + threadIdx.x), n = pp.g.n;
    const bool mine = k < n;
    const float Lx = pp.h.lis[0], Ly = pp.h.lis[1], Lz = pp.h.lis[2];
    const float4 p = pp.g.probes[mine ? k : 0];
    const Leg l = leg_between(Lx, Ly, Lz, p.x, p.y, p.z);
    const bool run = mine && l.w <= pp.max_attach && l.w != 0.0f;   // own actor {lo}
    const int end = path_chain(sc, pp.h, FS_NO_OBJECT, run, Lx, Ly, Lz, l.dx, l.dy, l.dz, l.w, stack, StopAtHit{});
    if (mine) pp.g.dL[k] = l.w > pp.max_attach ? INFINITY : (l.w == 0.0f ? 0.0f : (end == kChainReached ? l.w : INFINITY));
}

__global__ __launch_bounds__(kRelaxBlock) void pathing_relax_kernel(PathingSet g, float max_length) {
    __shared__ float s_px[kMaxProbes], s_py[kMaxProbes], s_pz[kMaxProbes], s_dL[kMaxProbes], s_d[2 * kMaxProbes];
    const int tid = (int)threadIdx.x, n = g.n;
    for (int i = tid; i < n; i += kRelaxBlock) {
        const float4 p = g.probes[i];
        const float dL = g.dL[i];
        s_px[i] = p.x; s_py[i] = p.y; s_pz[i] = p.z;
        s_d[i] = dL; s_dL[i] = dL;
    }
    __syncthreads();
    // Jacobi rounds between the two d arrays: a round reads one and writes every entry of the other, so the vote on "changed" is its
    // only barrier
    int cur = 0;
#pragma unroll 1
    for (int round = 0; round < n; ++round) {   // the hard cap: the fixed point is reached within n rounds, no input can make this spin
        const float* d = s_d + cur * kMaxProbes;
        float* next = s_d + (cur ^ 1) * kMaxProbes;
        bool changed = false;
#pragma unroll 1
        for (int i = tid; i < n; i += kRelaxBlock) {
            const float have = d[i], xi = s_px[i], yi = s_py[i], zi = s_pz[i];
            float best = have;   // (d only falls: min(dL[i], ...) and min(d[i], ...) are the same number)
            for_each_neighbour(g, i, [&](int j) {
                const float ex = s_px[j] - xi, ey = s_py[j] - yi, ez = s_pz[j] - zi;
                const float c = d[j] + sqrtf((ex * ex + ey * ey) + ez * ez);
                if (c <= max_length && c < best) best = c;
            });
            next[i] = best;
            changed = changed || best != have;
        }
        cur ^= 1;
        if (__syncthreads_or(changed ? 1 : 0) == 0) break;
    }
    const float* d = s_d + cur * kMaxProbes;
#pragma unroll 1
    for (int i = tid; i < n; i += kRelaxBlock) {   // pred: the listener, or the smallest neighbour that gives d[i]
        const float di = d[i], xi = s_px[i], yi = s_py[i], zi = s_pz[i];
        uint32_t pred = kListener;
        if (di != s_dL[i])
            for_each_neighbour(g, i, [&](int j) {
                const float ex = s_px[j] - xi, ey = s_py[j] - yi, ez = s_pz[j] - zi;
                const float c = d[j] + sqrtf((ex * ex + ey * ey) + ez * ez);
                if (c <= max_length && c == di && (uint32_t)j < pred) pred = (uint32_t)j;
            });
        g.d[i] = di;
        g.pred[i] = pred;
    }
}

__global__ __launch_bounds__(kBlock) void pathing_sources_kernel(DeviceScene sc, PathingKParams pp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] | keys [kBlock] | path [kMaxProbes] | direct, hops
    int* stack = &s_dyn[threadIdx.x];
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_dyn + (size_t)sc.stack_rows * kBlock);
    uint32_t* s_path = reinterpret_cast<uint32_t*>(s_key + kBlock);
    uint32_t* s_word = s_path + kMaxProbes;   // [0]: the DIRECT ray reached; [1]: hops
    const int tid = (int)threadIdx.x, lane = tid & 63, n = pp.g.n, row = (int)blockIdx.x, B = pp.h.num_bands;
    const float4 s4 = pp.h.src[row];
    const uint32_t so = __float_as_uint(s4.w);
    const float Lx = pp.h.lis[0], Ly = pp.h.lis[1], Lz = pp.h.lis[2];
    const float distance = row_distance(s4, pp.h.lis);
    if (tid == 0) { s_word[0] = 0u; s_word[1] = 0u; }
    __syncthreads();
    unsigned long long key = kNoKey;
#pragma unroll 1
    for (int base = 0; base < n + 1; base += kBlock) {   // (wave-uniform) index n is the DIRECT ray, towards the listener
        const int k = base + tid;
        const bool probe = k < n, direct = k == n;
        const float4 p = pp.g.probes[probe ? k : 0];
        const float dk = probe ? pp.g.d[k] : INFINITY;
        const Leg l = leg_between(s4.x, s4.y, s4.z, direct ? Lx : p.x, direct ? Ly : p.y, direct ? Lz : p.z);
        const bool wanted = direct || (dk < INFINITY && l.w <= pp.max_attach);
        const bool run = wanted && l.w != 0.0f;
        const int end = path_chain(sc, pp.h, so, run, s4.x, s4.y, s4.z, l.dx, l.dy, l.dz, direct ? l.w - pp.h.pullback : l.w, stack, StopAtHit{});
        const bool ok = wanted && (l.w == 0.0f || end == kChainReached);
        if (direct && ok) s_word[0] = 1u;
        if (probe && ok) {
            const float total = dk + l.w;
            if (total <= pp.max_length) key = min(key, ((unsigned long long)__float_as_uint(total) << 32) | (unsigned long long)(uint32_t)k);
        }
    }
    s_key[tid] = key;
    __syncthreads();
    for (int stride = kBlock / 2; stride > 0; stride >>= 1) {   // the smallest (total bits, k): a fixed tree
        if (tid < stride) s_key[tid] = min(s_key[tid], s_key[tid + stride]);
        __syncthreads();
    }
    key = s_key[0];
    if (tid == 0 && key != kNoKey) {   // follow pred to the listener: at most n probes
        uint32_t hops = 0u, cur = (uint32_t)key;
        for (int h = 0; h < n && cur != kListener; ++h) {
            s_path[hops++] = cur;
            cur = pp.g.pred[cur];
        }
        s_word[1] = hops;
    }
    __syncthreads();
    if (tid >= 64) return;   // the row is wave 0's
    uint32_t* words = reinterpret_cast<uint32_t*>(pp.out + row);
    const uint32_t direct_flag = s_word[0] != 0u ? FS_PATHING_DIRECT : 0u;
    if (key == kNoKey) {
        if (lane < kRowWords) words[lane] = lane == 3 ? __float_as_uint(distance) : (lane == 11 ? direct_flag : 0u);
        return;
    }
    const int hops = (int)s_word[1];
    bool stale = false;
    if (pp.validate != 0) {
        const PathKHead hb = no_actors(pp.h);
#pragma unroll 1
        for (int base = 0; base < hops - 1; base += 64) {   // (wave-uniform) the baked legs again, from the lower index
            const int m = base + lane;
            const bool have = m < hops - 1;
            const uint32_t a = s_path[have ? m : 0], b = s_path[have ? m + 1 : 0];
            const float4 lo = pp.g.probes[min(a, b)], hi = pp.g.probes[max(a, b)];
            const Leg l = leg_between(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
            const int end = path_chain(sc, hb, FS_NO_OBJECT, have, lo.x, lo.y, lo.z, l.dx, l.dy, l.dz, l.w, stack, StopAtHit{});
            stale = stale || __ballot(have && end != kChainReached) != 0ull;
        }
    }
    fs_pathing_path* o = pp.out + row;
    if (lane < FS_MAX_PATHING_NODES) o->probes[lane] = lane < hops ? s_path[hops - 1 - lane] : FS_PATHING_NO_PROBE;
    const float total = __uint_as_float((uint32_t)(key >> 32)), detour = total - distance;
    if (lane < FS_MAX_BANDS) o->gain[lane] = lane < B ? 1.0f / sqrtf(3.0f + pp.k[lane] * detour) : 0.0f;
    if (lane != 0) return;
    o->length = total;
    o->delay = path_delay(pp.h, total);
    o->detour = detour;
    o->distance = distance;
    // the first point at a distance from L along (n_0, ..., n_{hops-1}, S), and from S along (n_{hops-1}, ..., n_0, L)
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        const float fx = side ? s4.x : Lx, fy = side ? s4.y : Ly, fz = side ? s4.z : Lz;
        float ux = 0.0f, uy = 0.0f, uz = 0.0f;
        for (int q = 0; q <= hops; ++q) {
            float4 p = side ? make_float4(Lx, Ly, Lz, 0.0f) : s4;
            if (q < hops) p = pp.g.probes[s_path[side ? q : hops - 1 - q]];
            const Leg l = leg_between(fx, fy, fz, p.x, p.y, p.z);
            if (l.w != 0.0f) { ux = l.dx; uy = l.dy; uz = l.dz; break; }
        }
        float* u = side ? o->departure : o->direction;
        u[0] = ux; u[1] = uy; u[2] = uz;
    }
    o->hops = (uint32_t)hops;
    o->flags = FS_PATHING_FOUND | direct_flag | (stale ? FS_PATHING_STALE : 0u);
    o->first_probe = s_path[hops - 1];
    o->last_probe = s_path[0];
}

}  // namespace

void launch_pathing_bake(const DeviceScene& sc_in, const PathingBakeKParams& bp, hipStream_t s) {
    const int n = bp.g.n, nb = (n + 63) / 64;
    if (n <= 0) return;
    long long tasks = 0;
    for (int ib = 0; ib < nb; ++ib) tasks += (long long)std::min(64, n - ib * 64) * (nb - ib);
    const uint32_t blocks = (uint32_t)((tasks + kRowsPerBlock - 1) / kRowsPerBlock);
    DeviceScene sc = sc_in;
    if (!attach_deep(sc, blocks)) return;
    allow_lds(pathing_bake_kernel, stack_bytes(sc));
    hipLaunchKernelGGL(pathing_bake_kernel, dim3(blocks), dim3(kBlock), stack_bytes(sc), s, sc, bp);
    hipLaunchKernelGGL(pathing_mirror_kernel, dim3((uint32_t)((n * bp.g.stride + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, bp.g);
}

void launch_pathing_paths(const DeviceScene& sc_in, const PathingKParams& pp, hipStream_t s) {
    if (pp.h.count <= 0 || pp.g.n <= 0) return;
    DeviceScene sc = sc_in;
    const uint32_t attach_blocks = (uint32_t)((pp.g.n + kBlock - 1) / kBlock);
    if (!attach_deep(sc, std::max(attach_blocks, (uint32_t)pp.h.count))) return;
    const size_t lds_sources = stack_bytes(sc) + kSourcesLds;
    allow_lds(pathing_attach_kernel, stack_bytes(sc));
    hipLaunchKernelGGL(pathing_attach_kernel, dim3(attach_blocks), dim3(kBlock), stack_bytes(sc), s, sc, pp);
    hipLaunchKernelGGL(pathing_relax_kernel, dim3(1), dim3(kRelaxBlock), 0, s, pp.g, pp.max_length);
    allow_lds(pathing_sources_kernel, lds_sources);
    hipLaunchKernelGGL(pathing_sources_kernel, dim3((uint32_t)pp.h.count), dim3(kBlock), lds_sources, s, sc, pp);
}

}  // namespace fs
