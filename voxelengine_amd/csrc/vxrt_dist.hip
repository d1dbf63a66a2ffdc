// vxrt_dist.hip -- exact squared distance fields over a box of the resident brickmap (include/vxrt.h, vxrt_distance_field;
// host side in vxrt_api.hip, the shared logic in vxrt_dist.hpp).  A field is these launches on the caller's stream:
//
//   k_read_region   (vxrt_region.hip, unchanged) the halo's bits into the workspace.
//   k_dist_occ      one lane per occupancy cell (one halo word x 8 rows x 8 slices): some target in it.
//   k_dist_tiles    one 256-lane workgroup per tile of B (64^3): some occupied cell in the tile grown by R.
//   k_dist_ysweep   one workgroup per (64 columns of x, 64 rows of y, one halo slice) that a live tile reads: the x
//                   distances of min(64 + 2R, rows left) halo rows from the bits into an LDS slab (lanes along x, one wave
//                   per row in turn), then per output row the outward scan over the slab; g2 written as uint16 rows.
//   k_dist_zsweep   one workgroup per (64 columns of x, 8 rows of y, 64 slices of z): per row the slab of g2 slices, the
//                   same scan, the uint16 output; a tile that is not live is filled with FAR.  The summary is tallied per
//                   lane, reduced per wave and per workgroup, and added with one atomic per counter and workgroup.
//
// The slab is static LDS in three sizes (R <= 32: 16 KiB, R <= 96: 32 KiB, else 73.5 KiB of the CU's 160), so that a small
// radius keeps eight workgroups on a CU.  A slab row is 64 uint16: a wave reads and writes 128 contiguous bytes, two lanes
// per bank and no two addresses on one bank.
#include "../../include/vxrt.h"
#include "vxrt_dist.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_distance_summary) == 24, "distance summary layout");
static_assert(kDistTile == 64 && kDistTile % kDistRows == 0, "a slab row is one wave wide");

__global__ __launch_bounds__(256) void k_dist_occ(const DistArgs A, uint64_t n)
{
    const uint64_t i = flat_thread();
    if (i >= n)
        return;
    const uint64_t q = i / A.wh;
    dist_occ_cell(A, (uint32_t)(i % A.wh), (uint32_t)(q % A.ncy), (uint32_t)(q / A.ncy));
}

__global__ __launch_bounds__(256) void k_dist_tiles(const DistArgs A)
{
    const bool any = __syncthreads_or(dist_tile_part(A, blockIdx.x, threadIdx.x, 256u));
    if (threadIdx.x == 0)
        dist_tile_store(A, blockIdx.x, any);
}

template <uint32_t kSlabRows>
__global__ __launch_bounds__(256) void k_dist_ysweep(const DistArgs A)
{
    __shared__ uint16_t slab[kSlabRows * kDistTile];
    const uint64_t g = flat_block();
    if (g >= (uint64_t)A.ntx * A.nty * A.hz)
        return;
    const uint32_t tx = (uint32_t)(g % A.ntx), ty = (uint32_t)(g / A.ntx % A.nty), hz = (uint32_t)(g / A.ntx / A.nty);
    if (!dist_slice_live(A, tx, ty, hz))
        return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t left = A.hy - ty * kDistTile, rows = left < kDistTile + 2u * A.r ? left : kDistTile + 2u * A.r;
    for (uint32_t r = wave; r < rows; r += 4u)
        dist_y_load(A, slab, tx, ty, hz, r, lane);
    __syncthreads();
    for (uint32_t j = wave; j < kDistTile && ty * kDistTile + j < (uint32_t)A.d[1]; j += 4u)
        dist_y_store(A, slab, tx, ty, hz, j, lane);
}

template <uint32_t kSlabRows>
__global__ __launch_bounds__(256) void k_dist_zsweep(const DistArgs A, uint32_t nyc)
{
    __shared__ uint16_t slab[kSlabRows * kDistTile];
    __shared__ DistTally part[4];
    const uint64_t g = flat_block();
    if (g >= (uint64_t)A.ntx * nyc * A.ntz)
        return;
    const uint32_t tx = (uint32_t)(g % A.ntx), yc = (uint32_t)(g / A.ntx % nyc), tz = (uint32_t)(g / A.ntx / nyc);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool live = A.live[tx + A.ntx * (yc * kDistRows / kDistTile + A.nty * tz)] != 0;
    const uint32_t left = A.hz - tz * kDistTile, rows = left < kDistTile + 2u * A.r ? left : kDistTile + 2u * A.r;
    DistTally t{};
    for (uint32_t y = yc * kDistRows; y < (yc + 1u) * kDistRows && y < (uint32_t)A.d[1]; ++y) {
        if (live) {
            for (uint32_t r = wave; r < rows; r += 4u)
                dist_z_load(A, slab, tx, y, tz, r, lane);
            __syncthreads();
        }
        for (uint32_t j = wave; j < kDistTile && tz * kDistTile + j < (uint32_t)A.d[2]; j += 4u)
            dist_z_store(A, live ? slab : nullptr, tx, y, tz, j, lane, t);
        if (live)
            __syncthreads();
    }
    t.zero = wave_sum(t.zero);
    t.near = wave_sum(t.near);
    t.far = wave_sum(t.far);
    t.max_d2 = wave_max(t.max_d2);
    t.sum = wave_sum(t.sum);
    if (lane == 0) {
        part[wave].zero = t.zero;
        part[wave].near = t.near;
        part[wave].far = t.far;
        part[wave].max_d2 = t.max_d2;
        part[wave].sum = t.sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            t.zero += part[w].zero;
            t.near += part[w].near;
            t.far += part[w].far;
            t.max_d2 = part[w].max_d2 > t.max_d2 ? part[w].max_d2 : t.max_d2;
            t.sum += part[w].sum;
        }
        if (t.zero)
            atomicAdd(A.summary + kDistSumZero, t.zero);
        if (t.near)
            atomicAdd(A.summary + kDistSumNear, t.near);
        if (t.far)
            atomicAdd(A.summary + kDistSumFar, t.far);
        if (t.max_d2)
            atomicMax(A.summary + kDistSumMax, t.max_d2);
        if (t.sum)
            atomicAdd((unsigned long long*)(A.summary + kDistSumSum), (unsigned long long)t.sum);
    }
}

template <uint32_t kSlabRows>
static void dist_sweeps(const DistArgs& A, hipStream_t stream)
{
    const uint32_t nyc = ((uint32_t)A.d[1] + kDistRows - 1u) / kDistRows;
    hipLaunchKernelGGL(k_dist_ysweep<kSlabRows>, grid_2d((uint64_t)A.ntx * A.nty * A.hz), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_dist_zsweep<kSlabRows>, grid_2d((uint64_t)A.ntx * nyc * A.ntz), dim3(256), 0, stream, A, nyc);
}

// host entry point (vxrt_api.hip): arguments validated there (dist_layout accepts them).  Asynchronous on `stream`.
hipError_t distance_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t radius, uint32_t mode, void* work,
                          uint16_t* dist2, vxrt_distance_summary* summary, hipStream_t stream)
{
    DistLayout L;
    if (!dist_layout(o, d, radius, L))
        return hipErrorInvalidValue;
    DistArgs A{};
    dist_args(A, L, d, radius, mode, work, dist2, (uint32_t*)summary);
    hipError_t e;
    if ((e = hipMemsetAsync(summary, 0, sizeof(vxrt_distance_summary), stream)) != hipSuccess)
        return e;
    if ((e = read_region(W, L.ho, L.hd, (uint32_t*)((char*)work + L.halo), stream)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_dist_occ, grid_2d((L.nocc + 255u) / 256u), dim3(256), 0, stream, A, L.nocc);
    hipLaunchKernelGGL(k_dist_tiles, dim3(L.ntiles), dim3(256), 0, stream, A);
    if (radius <= 32u)
        dist_sweeps<kDistTile + 64u>(A, stream);
    else if (radius <= 96u)
        dist_sweeps<kDistTile + 192u>(A, stream);
    else
        dist_sweeps<kDistTile + 2u * kDistMaxRadius>(A, stream);
    return hipGetLastError();
}

}  // namespace vxrt
