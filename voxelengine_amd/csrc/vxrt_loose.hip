// vxrt_loose.hip -- loose voxels over a box of the resident brickmap (include/vxrt.h, vxrt_loose_step; host side in
// vxrt_api_query.hip, the shared logic in vxrt_loose.hpp).  A call is these launches on the caller's stream, their number
// fixed by the arguments alone (no host synchronisation, no grid-wide barrier: a pass is a launch):
//
//   k_read_region   (vxrt_region.hip, unchanged) the halo's solid bits into the blocked plane.
//   k_loose_setup   one lane per plane word: under VXRT_LOOSE_WALL the voxels outside Live ORed into the blocked plane, the
//                   live plane built, the input layer funnel-shifted to its bit offset in the halo's words and cut to
//                   Live & ~blocked into the first turn plane; the first lanes initialise the summary.
//   k_loose_pass    `steps` times two (sand) or three (water) launches, one lane per plane word, lanes along the words of a
//                   row: the layer words of the pass's stencil first and, when they are all zero, a zero stored and nothing
//                   of the blocked plane loaded (most of a box holds no loose material); else the word's movers and arrivals
//                   from word operations (vxrt_loose.hpp), the new word stored into the other of two planes.  The launches
//                   of the last step also count their movers (TALLY): a wave sum, one atomic per workgroup, none when zero.
//   k_loose_output  one lane per word of the layer, grid-stride: the input word read, L_n and the blocked plane funnel-shifted
//                   out of the halo's words and cut to the world voxels of B; L_n stored; the counts and the changed box summed
//                   per lane, then per wave, then per workgroup; one atomic per counter and workgroup.
#include <cstddef>

#include "../../include/vxrt.h"
#include "vxrt_loose.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_loose_summary) == 4u * kLooseSumWords, "loose summary layout");
static_assert(offsetof(vxrt_loose_summary, fell_last) == 4u * kLooseSumFell, "loose summary layout");
static_assert(offsetof(vxrt_loose_summary, spread_last) == 4u * kLooseSumSpread, "loose summary layout");
static_assert(offsetof(vxrt_loose_summary, changed_min) == 4u * kLooseSumMin, "loose summary layout");
static_assert(offsetof(vxrt_loose_summary, changed_max) == 4u * kLooseSumMax, "loose summary layout");
static_assert(sizeof(vxrt_loose) == 32, "loose layout");
static_assert(VXRT_LOOSE_MAX_STEPS == kLooseMaxSteps, "loose limits");
static_assert(VXRT_LOOSE_SAND == kLooseSand && VXRT_LOOSE_WATER == kLooseWater, "loose materials");
static_assert(VXRT_LOOSE_WALL == kLooseWall && VXRT_LOOSE_OPEN == kLooseOpen, "loose edges");
static_assert(kLooseSumFell + kLooseSlide == kLooseSumSlid && kLooseSumFell + kLooseSpread == kLooseSumSpread, "a pass's counter");

__global__ __launch_bounds__(256) void k_loose_setup(const LooseArgs A)
{
    const uint64_t i = flat_thread();
    if (i < kLooseSumWords)
        A.summary[i] = loose_summary_init((uint32_t)i);
    if (i < A.np)
        loose_setup_lane(A, i);
}

template <int PASS, bool TALLY>
__global__ __launch_bounds__(256) void k_loose_pass(const LooseArgs A, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t t)
{
    const uint64_t i = flat_thread();
    uint32_t n = 0u;
    if (i < A.np)
        n = loose_pass_lane<PASS, true>(A, src, dst, i, t);
    if (TALLY) {
        __shared__ uint32_t part[4];
        const uint32_t v = wave_sum(n);
        if ((threadIdx.x & 63u) == 0u)
            part[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0u) {
            const uint32_t sum = part[0] + part[1] + part[2] + part[3];
            if (sum)
                atomicAdd(A.summary + kLooseSumFell + PASS, sum);
        }
    }
}

__global__ __launch_bounds__(256) void k_loose_output(const LooseArgs A, const uint32_t* __restrict__ last)
{
    __shared__ uint32_t part[4][9];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    LooseTally t;
    loose_tally_clear(t);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < A.nb; i += (uint64_t)gridDim.x * 256u)
        loose_output_lane(A, last, i, t);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        const uint32_t v = wave_sum(t.n[k]);
        const int32_t lo = wave_min(t.lo[k]), hi = wave_max(t.hi[k]);
        if (lane == 0u) {
            part[wave][k] = v;
            part[wave][3u + k] = (uint32_t)lo;
            part[wave][6u + k] = (uint32_t)hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 9u) {
        const uint32_t k = threadIdx.x;
        if (k < 3u) {
            const uint32_t v = part[0][k] + part[1][k] + part[2][k] + part[3][k];
            if (v)
                atomicAdd(A.summary + kLooseSumIn + k, v);
        } else {
            int32_t v = (int32_t)part[0][k];
            for (uint32_t w = 1; w < 4u; ++w) {
                const int32_t o = (int32_t)part[w][k];
                v = k < 6u ? (o < v ? o : v) : (o > v ? o : v);
            }
            int32_t* box = (int32_t*)A.summary;
            if (k < 6u) {
                if (v != INT32_MAX)
                    atomicMin(box + kLooseSumMin + (k - 3u), v);
            } else if (v != INT32_MIN) {
                atomicMax(box + kLooseSumMax + (k - 6u), v);
            }
        }
    }
}

template <int PASS>
static void loose_pass_launch(const LooseArgs& A, int32_t p, uint32_t t, bool tally, hipStream_t stream)
{
    const dim3 grid = grid_2d((A.np + 255u) / 256u), wg(256);
    if (tally)
        hipLaunchKernelGGL((k_loose_pass<PASS, true>), grid, wg, 0, stream, A, loose_src(A, p), loose_dst(A, p), t);
    else
        hipLaunchKernelGGL((k_loose_pass<PASS, false>), grid, wg, 0, stream, A, loose_src(A, p), loose_dst(A, p), t);
}

// host entry point (vxrt_api_query.hip): arguments validated there (loose_check and loose_layout accept them).  Asynchronous
// on `stream`.
hipError_t loose_step(const CollideWorld& W, const int32_t o[3], const int32_t d[3], const vxrt_loose& params, const uint32_t* loose_in,
                      void* work, uint32_t* loose_out, vxrt_loose_summary* summary, hipStream_t stream)
{
    LooseLayout L;
    if (loose_check(params) != 0 || !loose_layout(o, d, L))
        return hipErrorInvalidValue;
    LooseArgs A{};
    loose_args(A, L, W, o, d, params, loose_in, work, loose_out, (uint32_t*)summary);
    hipError_t e;
    if ((e = read_region(W, L.ho, L.hd, A.blocked, stream)) != hipSuccess)
        return e;
    const dim3 wg(256);
    hipLaunchKernelGGL(k_loose_setup, grid_2d((L.np + 255u) / 256u), wg, 0, stream, A);
    const int32_t per = loose_passes_per_step(params.material), n = loose_passes(params);
    for (int32_t p = 0; p < n; ++p) {
        const uint32_t t = loose_pass_step(params, p);
        const bool tally = p >= n - per;  // the last step's passes
        const int kind = loose_pass_kind(params.material, p);
        if (kind == kLooseFall)
            loose_pass_launch<kLooseFall>(A, p, t, tally, stream);
        else if (kind == kLooseSlide)
            loose_pass_launch<kLooseSlide>(A, p, t, tally, stream);
        else
            loose_pass_launch<kLooseSpread>(A, p, t, tally, stream);
    }
    // few workgroups, each lane taking several words in turn, for the reason given at k_rule_output's launch (vxrt_rule.hip):
    // every workgroup ends in up to 9 atomics on the same 9 words
    const uint64_t tb = (L.nb + 255u) / 256u, few = tb / 8u < 128u ? (tb < 128u ? tb : 128u) : tb / 8u;
    hipLaunchKernelGGL(k_loose_output, dim3((unsigned)(few < 1024u ? few : 1024u)), wg, 0, stream, A, loose_src(A, n));
    return hipGetLastError();
}

}  // namespace vxrt
