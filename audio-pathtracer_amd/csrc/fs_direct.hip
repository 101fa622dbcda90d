// fs_direct.hip — fs_update_direct_paths: distance, arrival time, visibility and per-band transmission of the direct sound of
// every source of a tick, in one launch.  The definitions (sample offsets, chain, the per-source rule) are those of
// include/frequensee.h, operation by operation; this file is their mapping onto the device.
//   One wave per source row, lane k = sample k; a workgroup of kBlock threads serves kBlock / 64 rows.  Each lane runs its
// two chains — the validity chain from the source's centre to its sample point, then the chain towards the listener — with
// path_chain (fs_dev_paths.hpp), the loop the reflection and diffraction legs run too: the whole wave meets at every query, a lane
// whose chain has ended or whose sample does not exist idles along with an empty cursor.
//   Dynamic LDS: the stack rows [stack_rows][kBlock] | T [kBlock][FS_MAX_BANDS] | flags [kBlock].  The reduction has a
// fixed order: lane b of the row's wave adds the valid samples' T_k[b] serially in double, ascending k.
#include "fs_dev_paths.hpp"

namespace fs {
namespace {

constexpr uint32_t kDirectValid = 1u, kDirectFree = 2u;
constexpr size_t kDirectLdsBytes = (size_t)kBlock * (sizeof(float) * FS_MAX_BANDS + sizeof(uint32_t));

// chain(o, d, len) with the header's counting rule (path_chain, fs_dev_paths.hpp); `active` = this lane has a chain to run.
// T of a lane without one stays 1, crossed 0, reached false.
__device__ __forceinline__ void direct_chain(const DeviceScene& sc, const DirectKParams& dp, int max_surfaces, uint32_t src_object,
                                             bool active, float ox, float oy, float oz, float dx, float dy, float dz, float len,
                                             int* stack, bool& reached, uint32_t& crossed, float (&T)[FS_MAX_BANDS]) {
    const int B = dp.h.num_bands;
#pragma unroll
    for (int b = 0; b < FS_MAX_BANDS; ++b) T[b] = 1.0f;
    crossed = 0u;
    const int end = path_chain(sc, dp.h, src_object, active, ox, oy, oz, dx, dy, dz, len, stack,
                               [&](int leaf, float, float, float, float, float, float, float, float) {
        const uint32_t mat = __float_as_uint(sc.tris[leaf].c.y);
        crossed += 1u;
        bool through = false;
        if (crossed <= (uint32_t)max_surfaces) {
            const float* tau = sc.lobe_gain != nullptr && mat < (uint32_t)sc.num_materials
                                   ? sc.lobe_gain + ((size_t)mat * 3 + kLobeTransmit) * B : nullptr;
#pragma unroll
            for (int b = 0; b < FS_MAX_BANDS; ++b) {
                if (b < B) {
                    T[b] = T[b] * (tau != nullptr ? tau[b] : 0.0f);
                    through = through || T[b] != 0.0f;
                }
            }
        }
        return through;   // false: more surfaces than allowed, or nothing left in any band
    });
    reached = end == kChainReached;
    if (end == kChainStopped || end == kChainSpent) {   // blocked
#pragma unroll
        for (int b = 0; b < FS_MAX_BANDS; ++b) T[b] = 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void direct_paths_kernel(DeviceScene sc, DirectKParams dp) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];   // [stack_rows][kBlock] | T [kBlock][FS_MAX_BANDS] | flags [kBlock]
    int* stack = &s_dyn[threadIdx.x];
    float* s_t = reinterpret_cast<float*>(s_dyn + (size_t)sc.stack_rows * kBlock);
    uint32_t* s_flags = reinterpret_cast<uint32_t*>(s_t + (size_t)kBlock * FS_MAX_BANDS);
    const int lane = (int)(threadIdx.x & 63u), wbase = (int)(threadIdx.x & ~63u);
    const int row = (int)(blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6));
    const bool row_ok = row < dp.h.count;
    const int n = dp.samples, B = dp.h.num_bands;
    const bool mine = row_ok && lane < n;
    const float4 s4 = dp.h.src[row_ok ? row : 0];
    const uint32_t src_object = __float_as_uint(s4.w);
    const int k = mine ? lane : 0;
    const float ux = dp.offsets[3 * k], uy = dp.offsets[3 * k + 1], uz = dp.offsets[3 * k + 2];
    const float rad = dp.radius;

    bool reached;
    uint32_t crossed;
    float T[FS_MAX_BANDS];
    // valid: nothing counted lies between the centre and the sample point (only crossed == 0 is asked: the chain may end at its first
    // counted surface, which is what max_surfaces = 0 makes it do)
    direct_chain(sc, dp, 0, src_object, mine && lane > 0, s4.x, s4.y, s4.z, ux, uy, uz, rad, stack, reached, crossed, T);
    const bool valid = mine && (lane == 0 || crossed == 0u);

    const float px = s4.x + rad * ux, py = s4.y + rad * uy, pz = s4.z + rad * uz;
    const float ex = dp.h.lis[0] - px, ey = dp.h.lis[1] - py, ez = dp.h.lis[2] - pz;
    const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
    const bool trace = valid && len != 0.0f;
    const float inv = 1.0f / (trace ? len : 1.0f);
    direct_chain(sc, dp, dp.max_surfaces, src_object, trace, px, py, pz, ex * inv, ey * inv, ez * inv, len - dp.h.pullback, stack,
                 reached, crossed, T);
    const bool is_free = valid && (!trace || (reached && crossed == 0u));   // (len == 0: free with T = 1, what an idle chain leaves)

#pragma unroll
    for (int b = 0; b < FS_MAX_BANDS; ++b) s_t[(size_t)threadIdx.x * FS_MAX_BANDS + b] = T[b];
    s_flags[threadIdx.x] = (valid ? kDirectValid : 0u) | (is_free ? kDirectFree : 0u);
    __syncthreads();
    if (!row_ok || lane >= FS_MAX_BANDS) return;
    uint32_t V = 0u, nfree = 0u;
    double sum = 0.0;
    for (int j = 0; j < n; ++j) {
        const uint32_t f = s_flags[wbase + j];
        if (f & kDirectValid) {
            V += 1u;
            nfree += (f >> 1) & 1u;
            sum += (double)s_t[(size_t)(wbase + j) * FS_MAX_BANDS + lane];
        }
    }
    fs_direct_path* o = dp.out + row;
    o->transmission[lane] = lane < B ? (float)(sum / (double)V) : 0.0f;
    if (lane == 0) {
        const float dx = dp.h.lis[0] - s4.x, dy = dp.h.lis[1] - s4.y, dz = dp.h.lis[2] - s4.z;
        const float distance = sqrtf((dx * dx + dy * dy) + dz * dz);
        o->distance = distance;
        o->delay = path_delay(dp.h, distance);
        o->visibility = (float)nfree / (float)V;
        o->surfaces = crossed;
        o->samples_valid = V;
    }
}

}  // namespace

void launch_direct_paths(const DeviceScene& sc_in, const DirectKParams& dp, hipStream_t s) {
    if (dp.h.count <= 0) return;
    const uint32_t blocks = row_blocks(dp.h.count);
    DeviceScene sc = sc_in;
    if (!attach_deep(sc, blocks)) return;
    const size_t lds = stack_bytes(sc) + kDirectLdsBytes;
    allow_lds(direct_paths_kernel, lds);
    hipLaunchKernelGGL(direct_paths_kernel, dim3(blocks), dim3(kBlock), lds, s, sc, dp);
}

}  // namespace fs
