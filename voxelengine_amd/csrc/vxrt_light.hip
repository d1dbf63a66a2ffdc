// vxrt_light.hip -- voxel light fields over a box of the resident brickmap (include/vxrt.h, vxrt_light_field; host side in
// vxrt_api.hip, the shared logic in vxrt_light.hpp).  A field is these launches on the caller's stream, their number fixed
// by the arguments and the world's height alone (no host synchronisation):
//
//   k_read_region     (vxrt_region.hip, unchanged) the halo's solid bits into the workspace.
//   k_light_above     sky: one lane per (halo word, halo slice, slab of 8 world rows above the halo): the rows' words from
//                     the tables, ORed into the "blocked above" mask.  Not launched when the halo reaches the world's top.
//   k_light_columns   one lane per (halo word, halo slice), lanes along the words of a row: down the halo's rows, solid bits
//                     to empty bits in place and, for the sky channel, the exposed plane S_15; exposed voxels of B counted.
//   k_light_classify  block: one lane per emitter: its class, counted per wave, and its record.
//   k_light_scatter   block: one lane per emitter: the used emitters of level k ORed into S_k (15 launches).
//   k_light_round     14 launches, one lane per plane word and channel, lanes along the words of a row: S_k+1 added to
//                     the bit-sliced level planes, S_k = dilate6(S_k+1) & empty stored.  The x carries and the four
//                     neighbouring rows are loads of words the neighbouring lanes and waves load too: L1 / L2 hits.
//   k_light_expand    one lane per four output bytes: the level planes of B to (sky << 4) | block, one dword store per lane,
//                     256 contiguous bytes per wave.
//   k_light_tally     one lane per halo word that holds voxels of B, grid-stride: per level the word's voxels by
//                     popcount, one channel at a time, summed per lane, then per wave, then per workgroup; one atomic
//                     per counter and workgroup.
#include <cstddef>

#include "../../include/vxrt.h"
#include "vxrt_light.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_light_summary) == 4u * kLightSumWords, "light summary layout");
static_assert(offsetof(vxrt_light_summary, hist_sky) == 4u * kLightSumHist, "light summary layout");
static_assert(offsetof(vxrt_light_summary, sum_sky) == 4u * kLightSumSum, "light summary layout");
static_assert(offsetof(vxrt_light_summary, emitters_used) == 4u * kLightSumUsed, "light summary layout");
static_assert(VXRT_LIGHT_MAX == kLightMax && VXRT_LIGHT_MAX_EMITTERS == kLightMaxEmitters, "light limits");

__global__ __launch_bounds__(256) void k_light_above(const LightArgs A, const CollideWorld W, int64_t first, uint64_t n)
{
    const uint64_t i = flat_thread();
    if (i < n)
        light_above_lane(A, W, first, i);
}

__global__ __launch_bounds__(256) void k_light_columns(const LightArgs A, uint64_t n)
{
    const uint64_t i = flat_thread();
    uint32_t count = i < n ? light_column_lane(A, i) : 0u;
    count = wave_sum(count);
    if ((threadIdx.x & 63u) == 0u && count)
        atomicAdd(A.summary + kLightSumExposed, count);
}

__global__ __launch_bounds__(256) void k_light_classify(const LightArgs A)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const uint32_t cls = e < A.n_emitters ? light_classify_lane(A, e) : 4u;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t n = (uint32_t)__popcll(__ballot(cls == k));
        if ((threadIdx.x & 63u) == 0u && n)
            atomicAdd(A.summary + kLightSumUsed + k, n);
    }
}

__global__ __launch_bounds__(256) void k_light_scatter(const LightArgs A, uint32_t* plane, uint32_t k)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e < A.n_emitters)
        light_scatter_lane(A, plane, k, e);
}

__global__ __launch_bounds__(256) void k_light_round(const LightArgs A, uint32_t turn, uint64_t n)
{
    const uint64_t i = flat_thread();
    if (i < n)
        light_round_lane(A, turn, i);
}

__global__ __launch_bounds__(256) void k_light_expand(const LightArgs A, uint64_t n)
{
    const uint64_t j = flat_thread();
    if (j < n)
        light_expand_lane(A, j);
}

__global__ __launch_bounds__(256) void k_light_tally(const LightArgs A, uint64_t n)
{
    __shared__ uint32_t part[4][33];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t ch = 0; ch < 2u; ++ch) {  // one channel at a time: 17 counters per lane
        LightTally t{};
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
            light_tally_lane(A, ch, i, t);
        if (ch == 0u) {
            const uint32_t solid = wave_sum(t.solid);
            if (lane == 0u)
                part[wave][32] = solid;
        }
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t v = wave_sum(t.hist[k]);
            if (lane == 0u)
                part[wave][16u * ch + k] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < 33u) {
        const uint32_t k = threadIdx.x, v = part[0][k] + part[1][k] + part[2][k] + part[3][k];
        if (v) {
            atomicAdd(A.summary + (k == 32u ? (uint32_t)kLightSumSolid : kLightSumHist + k), v);
            if (k < 32u && (k & 15u))
                atomicAdd((unsigned long long*)(A.summary + kLightSumSum) + (k >> 4), (unsigned long long)v * (k & 15u));
        }
    }
}

// host entry point (vxrt_api.hip): arguments validated there (light_layout accepts them).  Asynchronous on `stream`.
hipError_t light_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t channels, const int32_t* emitters,
                       uint32_t n_emitters, void* work, uint8_t* levels, vxrt_light_summary* summary, hipStream_t stream)
{
    LightLayout L;
    if (!light_layout(o, d, channels, L))
        return hipErrorInvalidValue;
    LightArgs A{};
    light_args(A, L, o, d, channels, work, emitters, n_emitters, levels, (uint32_t*)summary);
    hipError_t e;
    if ((e = hipMemsetAsync(summary, 0, sizeof(vxrt_light_summary), stream)) != hipSuccess)
        return e;
    if ((e = read_region(W, L.ho, L.hd, A.empty, stream)) != hipSuccess)
        return e;
    const dim3 wg(256);
    if (A.sky < 2u) {
        if ((e = hipMemsetAsync(A.above, 0, 4u * L.nabove, stream)) != hipSuccess)
            return e;
        const uint64_t n = L.nabove * light_above_slabs(A, W);
        if (n)
            hipLaunchKernelGGL(k_light_above, grid_2d((n + 255u) / 256u), wg, 0, stream, A, W, light_above_first(A), n);
    }
    hipLaunchKernelGGL(k_light_columns, grid_2d((L.nabove + 255u) / 256u), wg, 0, stream, A, L.nabove);
    const dim3 eg((A.n_emitters + 255u) / 256u);
    if (A.block < 2u) {
        if ((e = hipMemsetAsync(A.set[A.block][0], 0, 4u * L.np, stream)) != hipSuccess)
            return e;
        if (A.n_emitters) {
            hipLaunchKernelGGL(k_light_classify, eg, wg, 0, stream, A);
            hipLaunchKernelGGL(k_light_scatter, eg, wg, 0, stream, A, A.set[A.block][0], kLightMax);
        }
    }
    const uint64_t nr = L.np * L.nch;
    for (uint32_t turn = 0; turn < kLightMax - 1u; ++turn) {
        hipLaunchKernelGGL(k_light_round, grid_2d((nr + 255u) / 256u), wg, 0, stream, A, turn, nr);
        if (A.n_emitters)
            hipLaunchKernelGGL(k_light_scatter, eg, wg, 0, stream, A, A.set[A.block][~turn & 1u], kLightMax - 1u - turn);
    }
    const uint64_t ne = ((uint64_t)L.nvox + 3u) / 4u, nt = (uint64_t)light_box_words(A) * (uint32_t)d[1] * (uint32_t)d[2];
    hipLaunchKernelGGL(k_light_expand, grid_2d((ne + 255u) / 256u), wg, 0, stream, A, ne);
    // few workgroups, each lane taking several words in turn: every workgroup ends in up to 63 atomics on the same 36
    // counters, and with one workgroup per 256 words those atomics, not the words, were the kernel's time
    const uint64_t tb = (nt + 255u) / 256u, few = tb / 8u < 128u ? (tb < 128u ? tb : 128u) : tb / 8u;
    hipLaunchKernelGGL(k_light_tally, dim3((unsigned)(few < 1024u ? few : 1024u)), wg, 0, stream, A, nt);
    return hipGetLastError();
}

}  // namespace vxrt
