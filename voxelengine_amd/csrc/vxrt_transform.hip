// vxrt_transform.hip -- voxel stamps rotated and mirrored on the device (include/vxrt.h, vxrt_transform_stamp; host side in
// vxrt_api_query.hip, the shared logic in vxrt_transform.hpp).  A call is these launches on the caller's stream, fixed by the
// arguments alone (no host synchronisation, no allocation):
//
//   k_transform_init       (only with a summary) one wave writes the summary's eight words: no voxel, empty bounds.
//   k_transform_copy       axis[0] == 0: one lane per destination word, lanes along the words of a row, the workgroups
//                          walking the words with the launch's stride.  A copy with the row index permuted, one funnel
//                          shift and one bit reversal per word where x is flipped.
//   k_transform_transpose  axis[0] != 0: a workgroup per tile of 256 source rows by 16 x-words (16 KiB of bits), the
//                          workgroups walking the tiles with the launch's stride.  Load with lanes along source x, a padded
//                          LDS image, the 32 x 32 bit transpose of a half-wave in five __shfl_xor rounds, a second padded LDS
//                          image, store with lanes along destination x: global loads are contiguous in runs of 64 bytes and
//                          global stores in runs of 32, and the LDS column accesses are free of bank conflicts
//                          (vxrt_transform.hpp).  The butterfly is 5 shuffles and about 25 VALU operations per 32 words; the
//                          alternative, 32 ballots per 64 words, puts 32 wave-wide compares and 64-bit scalar moves on the
//                          scalar pipe for the same words and was not built.
//
// With a summary each lane tallies the words it stores; a workgroup reduces its lanes (xor shuffles, then LDS) and issues
// one atomic add, and a minimum or maximum only where the bound it reads is not as wide already: integer sums, minima and
// maxima, so the result does not depend on the order.  Atomics on one address are served one after the other, about 11 ns
// each here: one per wave and field cost 1.3 ms on a 1024^3 stamp, beside a kernel of 0.06 ms (profiles/r20_transform.md).
#include <cstddef>

#include "../../include/vxrt.h"
#include "vxrt_transform.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_orientation) == sizeof(Orient) && offsetof(vxrt_orientation, flip) == offsetof(Orient, flip), "orientation layout");
static_assert(sizeof(vxrt_transform_summary) == 4u * kTrSumWords, "transform summary layout");
static_assert(offsetof(vxrt_transform_summary, set_min) == 4u * kTrSumMin, "transform summary layout");
static_assert(offsetof(vxrt_transform_summary, set_max) == 4u * kTrSumMax, "transform summary layout");
static_assert(VXRT_TRANSFORM_MAX_WORDS == kTransformMaxWords, "transform limits");

__global__ __launch_bounds__(64) void k_transform_init(uint32_t* summary)
{
    if (threadIdx.x < kTrSumWords)
        summary[threadIdx.x] = tr_summary_init(threadIdx.x);
}

// the workgroup's tallies reduced -- xor shuffles within a wave, LDS across the four waves -- and committed by its first
// lane; every lane of the workgroup calls it
__device__ inline void transform_commit(const TransformArgs& A, const TrTally& t)
{
    __shared__ uint32_t part[kTrLanes / 64u][8];
    int32_t lo[3] = {t.lo[0], t.lo[1], t.lo[2]}, hi[3] = {t.hi[0], t.hi[1], t.hi[2]};
    uint64_t sum = t.n;  // (a lane's count fits 32 bits, a wave's need not: a lane can store 2^26 words)
    for (int m = 32; m; m >>= 1) {
        sum += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(sum >> 32), m, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)sum, m, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int32_t a = __shfl_xor(lo[k], m, 64), b = __shfl_xor(hi[k], m, 64);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        part[wave][0] = (uint32_t)sum;
        part[wave][1] = (uint32_t)(sum >> 32);
        for (int k = 0; k < 3; ++k) {
            part[wave][2 + k] = (uint32_t)lo[k];
            part[wave][5 + k] = (uint32_t)hi[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t v = 1; v < kTrLanes / 64u; ++v) {
            sum += ((uint64_t)part[v][1] << 32) | part[v][0];
            for (int k = 0; k < 3; ++k) {
                const int32_t a = (int32_t)part[v][2 + k], b = (int32_t)part[v][5 + k];
                lo[k] = a < lo[k] ? a : lo[k];
                hi[k] = b > hi[k] ? b : hi[k];
            }
        }
        tr_commit(A, sum, lo, hi);
    }
}

template <bool TALLY>
__global__ __launch_bounds__(256) void k_transform_copy(const TransformArgs A)
{
    TrTally t;
    tr_tally_clear(t);
    const uint64_t stride = (uint64_t)gridDim.x * kTrLanes;
    for (uint64_t w = (uint64_t)blockIdx.x * kTrLanes + threadIdx.x; w < A.ndst; w += stride)
        tr_copy_word(A, (uint32_t)w, TALLY, t);
    if (TALLY)
        transform_commit(A, t);
}

template <bool TALLY>
__global__ __launch_bounds__(256) void k_transform_transpose(const TransformArgs A)
{
    __shared__ uint32_t in[kTrLdsInWords], out[kTrLdsOutWords];
    const uint32_t lane = threadIdx.x, half = lane >> 5, i = lane & 31u;
    TrTally t;
    tr_tally_clear(t);
    for (uint64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {  // the same trip count in every lane of a workgroup
        const TrTile T = tr_tile(A, (uint32_t)tile);
        uint32_t v[kTrLoads];
#pragma unroll
        for (uint32_t e = 0; e < kTrLoads; ++e) {  // every load issued before the first LDS store
            uint32_t r, xl;
            tr_load_slot(lane, e, r, xl);
            v[e] = tr_load_word(A, T, r, xl);
        }
#pragma unroll
        for (uint32_t e = 0; e < kTrLoads; ++e) {
            uint32_t r, xl;
            tr_load_slot(lane, e, r, xl);
            in[tr_lds_in(r, xl)] = v[e];
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t b = 0; b < kTrBlocks; ++b) {
            uint32_t jl, xl;
            tr_block(half, b, jl, xl);
            uint32_t w = in[tr_lds_in(32u * jl + i, xl)];
#pragma unroll
            for (uint32_t round = 0; round < 5u; ++round)
                w = tr_combine(w, (uint32_t)__shfl_xor((int)w, (int)(16u >> round), 64), round, i);
            out[tr_lds_out(32u * xl + i, jl)] = tr_finish_word(A, w);
        }
        __syncthreads();  // (the next tile's stores into `in` come after this barrier, its stores into `out` after the next)
#pragma unroll
        for (uint32_t e = 0; e < kTrLoads; ++e) {
            uint32_t xrow, jl;
            tr_store_slot(lane, e, xrow, jl);
            tr_store_word(A, T, xrow, jl, out[tr_lds_out(xrow, jl)], TALLY, t);
        }
    }
    if (TALLY)
        transform_commit(A, t);
}

// host entry point (vxrt_api_query.hip): A from transform_plan with the pointers set, the ranges checked there.
// Asynchronous on `stream`.
hipError_t transform_stamp(const TransformArgs& A, hipStream_t stream)
{
    const bool tally = A.summary != nullptr;
    if (tally)
        hipLaunchKernelGGL(k_transform_init, dim3(1), dim3(64), 0, stream, A.summary);
    const dim3 grid(transform_groups(A)), wg(kTrLanes);
    if (A.axis[0] == 0) {
        if (tally)
            hipLaunchKernelGGL(k_transform_copy<true>, grid, wg, 0, stream, A);
        else
            hipLaunchKernelGGL(k_transform_copy<false>, grid, wg, 0, stream, A);
    } else if (tally) {
        hipLaunchKernelGGL(k_transform_transpose<true>, grid, wg, 0, stream, A);
    } else {
        hipLaunchKernelGGL(k_transform_transpose<false>, grid, wg, 0, stream, A);
    }
    return hipGetLastError();
}

}  // namespace vxrt
