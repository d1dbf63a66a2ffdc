// vxrt_place.hip -- voxel piece queries against the resident brickmap (include/vxrt.h, vxrt_place_pieces; host side in
// vxrt_api.hip, the per-lane logic in vxrt_place.hpp).
//
//   k_place_init     one lane per placement: the result's accumulators ({0, |dist| + 1, 0, 0}), or INVALID.
//   k_place_sweep    one lane per piece row: a task is (placement, chunk of `lanes` rows), `lanes` a power of two up to 64, so
//                    a wave holds 64 / lanes tasks -- 64 placements of a one-row piece, one chunk of a big one.  The lanes of a
//                    task add their rows' overlap at the origin, then test the steps nearest first together (x: 32 steps per
//                    64-bit window) and stop at the first blocked one; tasks of one placement meet in an atomic minimum and
//                    read it before every step, so a chunk high above the ground stops when a lower one has landed.
//   k_place_contact  the same lanes once more for blocked placements: the overlap at the first blocked step.
//   k_place_finish   one lane per placement: travel and flags.
// The results are the only accumulators (no workspace).  Minimum and integer sums are order-free, so the results do not
// depend on the grid or on scheduling.  Every gather is region_row_word on a row tested against the world first, and a piece
// is read inside its region words only.  The mapping and its costs: DESIGN.md 4.17.
#include "../../include/vxrt.h"
#include "vxrt_place.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_placement) == 24 && sizeof(vxrt_placed) == 16 && sizeof(vxrt_piece) == 24, "piece query layouts");
static_assert(sizeof(PlaceArgs) <= 4096, "the call travels as kernel arguments");

__global__ __launch_bounds__(256) void k_place_init(const PlaceArgs A)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += stride)
        place_init(A, i);
}

// one lane per (task, row): the grid holds every lane of the launch (grid_2d), so the task loop of a lane is one step
__global__ __launch_bounds__(256) void k_place_sweep(const PlaceArgs A, uint64_t n_tasks, uint32_t lg_lanes)
{
    const uint64_t t = flat_thread() >> lg_lanes;
    if (t < n_tasks)
        place_sweep(A, t, threadIdx.x & (A.lanes - 1u));
}

__global__ __launch_bounds__(256) void k_place_contact(const PlaceArgs A, uint64_t n_tasks, uint32_t lg_lanes)
{
    const uint64_t t = flat_thread() >> lg_lanes;
    if (t < n_tasks)
        place_contact(A, t, threadIdx.x & (A.lanes - 1u));
}

__global__ __launch_bounds__(256) void k_place_finish(const PlaceArgs A)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += stride)
        place_finish(A, i);
}

// up to 64 K workgroups of 256 lanes; a grid-stride loop covers larger batches
static unsigned place_blocks(uint64_t lanes)
{
    const uint64_t b = (lanes + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : (b ? b : 1));
}

// host entry point (vxrt_api.hip); A.n > 0, A.lanes / A.tasks set by place_shape.  A batch is cut into launches of at most
// 2^30 lanes (whole placements; a placement has at most 2^20 lanes), each with its own four kernels on the stream.
hipError_t place_pieces(const PlaceArgs& A0, hipStream_t stream)
{
    uint32_t lg = 0;
    while ((1u << lg) < A0.lanes)
        ++lg;
    const uint64_t per_placement = (uint64_t)A0.tasks << lg;
    const uint64_t most = ((1ull << 30) + per_placement - 1) / per_placement;
    for (uint64_t at = 0; at < A0.n; at += most) {
        PlaceArgs A = A0;
        A.placements += at * 6;
        A.results += at * 4;
        A.n = A0.n - at < most ? A0.n - at : most;
        const uint64_t n_tasks = A.n * A.tasks;
        const dim3 all = grid_2d(((n_tasks << lg) + 255) / 256);
        const unsigned per = place_blocks(A.n);
        hipLaunchKernelGGL(k_place_init, dim3(per), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(k_place_sweep, all, dim3(256), 0, stream, A, n_tasks, lg);
        hipLaunchKernelGGL(k_place_contact, all, dim3(256), 0, stream, A, n_tasks, lg);
        hipLaunchKernelGGL(k_place_finish, dim3(per), dim3(256), 0, stream, A);
    }
    return hipGetLastError();
}

}  // namespace vxrt
