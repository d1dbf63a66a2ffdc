// vxrt_lod.hip -- occupancy LOD of a box of the resident brickmap (include/vxrt.h, vxrt_downsample_region; host side in
// vxrt_api.hip, the shared logic in vxrt_lod.hpp).  A call is these launches on the caller's stream:
//
//   k_read_region   (vxrt_region.hip, unchanged) the source box's bits into the workspace.
//   k_lod_reduce    one lane per (source word column k, cell row (Y, Z)), a wave on 64 consecutive words of a row (or on
//                   64 / L short rows): the lane adds word k of the cell's f * f source rows in packed form
//                   (vxrt_lod.hpp), so every load of a wave is contiguous and the trip count is the same for every lane;
//                   it ends with the 32 / f counts of its word.  The f lanes of an output word OR their bits together with
//                   xor shuffles (at most five, once per lane after up to 1024 loads: the same path serves every shift, so
//                   shift 5 does not get a ballot of its own) and the group's first lane stores the word; counts go out as
//                   contiguous uint16.  No two lanes write the same word: no atomics on the outputs.
//                   A wave takes `iters` consecutive tasks in turn (16 at shift 1, 4 at shift 2, else 1), so that a lane
//                   loads about 64 words before the workgroup pays for its tally reduction.
//                   SPLIT (f >= 16 and fewer than 1024 tasks): the four waves of a workgroup share one task, each walks a
//                   quarter of the cell's z slices, waves 1 .. 3 leave their accumulators in LDS and wave 0 adds them and
//                   finishes.  It keeps four times the lanes in flight where the plain kernel would leave SIMDs idle.
//
// The summary is tallied per lane, reduced per wave and per workgroup, and added with one atomic per counter and workgroup
// onto the zeroed summary: integer sums and a maximum, so the result does not depend on the order.
#include "../../include/vxrt.h"
#include "vxrt_lod.hpp"

#include <cstdlib>

namespace vxrt {

static_assert(sizeof(vxrt_lod_summary) == 32, "lod summary layout");
static_assert(offsetof(vxrt_lod_summary, set) == 8 && offsetof(vxrt_lod_summary, max_count) == 24, "lod summary layout");

// the workgroup's tallies into the summary; every thread of the workgroup calls it
__device__ inline void lod_commit(const LodArgs& A, const LodTally& t)
{
    __shared__ uint32_t part[4][6];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t v[6] = {wave_sum(t.solid), wave_sum(t.set), wave_sum(t.empty), wave_sum(t.full), wave_sum(t.mixed),
                           wave_max(t.max_count)};
    if (lane == 0u)
        for (int i = 0; i < 6; ++i)
            part[wave][i] = v[i];
    __syncthreads();
    if (threadIdx.x < 6u) {
        const uint32_t a = part[0][threadIdx.x], b = part[1][threadIdx.x], c = part[2][threadIdx.x], d = part[3][threadIdx.x];
        vxrt_lod_summary* s = (vxrt_lod_summary*)A.summary;
        if (threadIdx.x == 5u) {
            const uint32_t m = max(max(a, b), max(c, d));
            if (m)
                atomicMax(&s->max_count, m);
        } else if (const uint32_t n = a + b + c + d) {  // a workgroup's solid voxels: at most 256 lanes x 32 x 1024 = 2^23
            if (threadIdx.x == 0u)
                atomicAdd((unsigned long long*)&s->solid, (unsigned long long)n);
            else
                atomicAdd(&s->set + (threadIdx.x - 1u), n);
        }
    }
}

template <uint32_t SH, bool SPLIT>
__global__ __launch_bounds__(256) void k_lod_reduce(const LodArgs A)
{
    __shared__ uint32_t part[SPLIT ? 3 : 1][64][2];
    constexpr uint32_t f = 1u << SH;
    const uint32_t b = (uint32_t)flat_block();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t iters = SPLIT ? 1u : A.iters, group = lod_group(A);  // SPLIT: one task, so one barrier per launch
    LodTally t{};
    for (uint32_t i = 0; i < iters; ++i) {  // the same trip count in every lane
        uint32_t k, row;
        const bool live = lod_lane(A, lod_wave_task(SPLIT ? b : 4u * b + wave, iters, i), lane, k, row);
        uint32_t lo = 0u, hi = 0u;
        if (live) {
            const uint32_t Y = row % (uint32_t)A.d[1], Z = row / (uint32_t)A.d[1];
            if (SPLIT)
                lod_accumulate<SH>(A, k, Y, Z, wave * (f / 4u), (wave + 1u) * (f / 4u), lo, hi);
            else
                lod_accumulate<SH>(A, k, Y, Z, 0u, f, lo, hi);
        }
        if (SPLIT) {
            if (wave) {
                part[wave - 1u][lane][0] = lo;
                part[wave - 1u][lane][1] = hi;
            }
            __syncthreads();
            if (!wave) {
                lo += part[0][lane][0] + part[1][lane][0] + part[2][lane][0];
                hi += part[0][lane][1] + part[1][lane][1] + part[2][lane][1];
            }
        }
        if (!SPLIT || !wave) {  // wave-uniform: every lane of a finishing wave takes part in the shuffles
            uint32_t word = live ? lod_finish<SH>(A, k, row, lo, hi, t) : 0u;
            for (uint32_t s = 1; s < group; s <<= 1)
                word |= (uint32_t)__shfl_xor((int)word, (int)s, 64);
            if (live)
                lod_store(A, k, row, word);
        }
    }
    lod_commit(A, t);
}

template <uint32_t SH>
static void lod_launch(const LodArgs& A, const LodLayout& L, bool split, hipStream_t stream)
{
    if constexpr (SH >= 3u) {
        if (split) {
            hipLaunchKernelGGL((k_lod_reduce<SH, true>), grid_2d(L.tasks), dim3(256), 0, stream, A);
            return;
        }
    }
    const uint32_t waves = (L.tasks + L.iters - 1u) / L.iters;
    hipLaunchKernelGGL((k_lod_reduce<SH, false>), grid_2d((waves + 3u) / 4u), dim3(256), 0, stream, A);
}

// host entry point (vxrt_api.hip): arguments validated there (lod_layout accepts them, 1 <= threshold <= f^3).
// Asynchronous on `stream`.
hipError_t downsample_region(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t shift, uint32_t threshold,
                             void* work, uint32_t* bits, uint16_t* counts, vxrt_lod_summary* summary, hipStream_t stream)
{
    LodLayout L;
    if (!lod_layout(o, d, shift, L))
        return hipErrorInvalidValue;
    LodArgs A{};
    lod_args(A, L, d, shift, threshold, work, bits, counts, summary);
    hipError_t e;
    if ((e = hipMemsetAsync(summary, 0, sizeof(vxrt_lod_summary), stream)) != hipSuccess)
        return e;
    if ((e = read_region(W, o, L.S, (uint32_t*)work, stream)) != hipSuccess)
        return e;
    // SPLIT where the plain kernel would leave SIMDs without a wave (256 CUs x 4) and a lane's walk is long enough to
    // quarter: measured a win at shift 5 with 64 tasks, even at shift 4 with 256, a loss from 1024 tasks on and at shift 3
    // (profiles/r14_lod.md)
    bool split = shift >= 4u && L.tasks < 1024u;
#ifdef VXRT_EXPERIMENTS
    if (const char* e = getenv("VXRT_LOD_SPLIT"))  // tools/lod_probe.py: 0 = the plain kernel, 1 = SPLIT wherever it exists
        split = shift >= 3u && e[0] != '0';
#endif
    switch (shift) {
    case 1: lod_launch<1>(A, L, false, stream); break;
    case 2: lod_launch<2>(A, L, false, stream); break;
    case 3: lod_launch<3>(A, L, split, stream); break;
    case 4: lod_launch<4>(A, L, split, stream); break;
    default: lod_launch<5>(A, L, split, stream); break;
    }
    return hipGetLastError();
}

}  // namespace vxrt
