// vxrt_surface.hip -- surface quads and triangles of a box of the resident brickmap (include/vxrt.h, vxrt_extract_surface;
// host side in vxrt_api.hip, the shared logic in vxrt_surface.hpp).  An extraction is these launches on the caller's stream:
//
//   k_read_region    (vxrt_region.hip, unchanged) the halo's bits into the workspace.
//   k_surf_count_yz  one lane per row (d, s, v) of the y and z directions, consecutive lanes on consecutive rows v: the
//                    face words of the row, its run starts by word operations, per run the identical-run test against
//                    row v - 1; the row's quad count; the solid voxels (by the rows of -y) and the faces.
//   k_surf_count_x   one lane per (d, z, x) of the x directions, the 64 lanes of a wave on 64 consecutive slices x of one
//                    row z: every lane walks y with the same trip count and the wave's loads fall into two or three
//                    words per step; the count goes to row (d, x, z).
//   k_surf_scan      one lane per row: the exclusive scan of 256 counts (wave shuffles, then the four waves' totals)
//                    in place, and the group's total.
//   k_surf_groups    one workgroup: the exclusive scan of the group totals, every lane a contiguous share; the
//                    summary's totals and `written`.
//   k_surf_emit_yz, k_surf_emit_x   the count passes' lane mappings again: a row whose first index is below the capacity
//                    finds its quad starts again, walks down for h and writes records, vertices and triangles.
//
// No atomic decides a position: a quad's index is its row's scanned count plus its rank within the row.  The summary is
// tallied per lane, reduced per wave and per workgroup, and added with one atomic per counter and workgroup.
#include "../../include/vxrt.h"
#include "vxrt_surface.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_surface_summary) == 64, "surface summary layout");
static_assert(sizeof(vxrt_quad) == 8, "quad record layout");
static_assert(kSurfGroup == 256, "the scan's group is one workgroup");

// the workgroup's tallies by direction into the summary; every thread of the workgroup calls it
__device__ inline void surf_commit(const SurfArgs& A, const SurfTally& t, uint32_t dir, bool live)
{
    __shared__ uint32_t part[4][13];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t solid = wave_sum(live ? t.solid : 0u);
    if (lane == 0u)
        part[wave][12] = solid;
    for (uint32_t d = 0; d < 6u; ++d) {
        const uint32_t f = wave_sum(live && dir == d ? t.faces : 0u), q = wave_sum(live && dir == d ? t.quads : 0u);
        if (lane == 0u) {
            part[wave][d] = f;
            part[wave][6u + d] = q;
        }
    }
    __syncthreads();
    if (threadIdx.x < 13u) {
        const uint32_t n = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (n)
            atomicAdd(A.summary + (threadIdx.x == 12u ? (uint32_t)kSurfSumSolid : (uint32_t)kSurfSumFacesDir + threadIdx.x), n);
    }
}

__global__ __launch_bounds__(256) void k_surf_count_yz(const SurfArgs A)
{
    const uint32_t j = (uint32_t)flat_block() * 256u + threadIdx.x;
    SurfTally t{};
    uint32_t dir = 0u;
    if (j < A.nryz)
        A.counts[A.nrx + j] = surf_row_yz<false>(A, j, 0u, t, dir);
    surf_commit(A, t, dir, j < A.nryz);
}

// lane i: x = i % x64, z = i / x64 % dims[2], d = i / x64 / dims[2], with x64 = dims[0] rounded up to whole waves
__global__ __launch_bounds__(256) void k_surf_count_x(const SurfArgs A, uint32_t x64)
{
    const uint32_t i = (uint32_t)flat_block() * 256u + threadIdx.x;
    const uint32_t x = i % x64, q = i / x64, z = q % (uint32_t)A.d[2], d = q / (uint32_t)A.d[2];
    const bool live = d < 2u && x < (uint32_t)A.d[0];
    SurfTally t{};
    if (live)
        A.counts[surf_row_index_x(A, d, (int32_t)x, (int32_t)z)] = surf_row_x<false>(A, d, (int32_t)x, (int32_t)z, 0u, t);
    surf_commit(A, t, d, live);
}

__global__ __launch_bounds__(256) void k_surf_scan(const SurfArgs A)
{
    __shared__ uint32_t part[4];
    const uint32_t i = (uint32_t)flat_block() * kSurfGroup + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t count = i < A.nrows ? A.counts[i] : 0u;
    uint32_t incl = count;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, s, 64);
        incl += lane >= (uint32_t)s ? o : 0u;
    }
    if (lane == 63u)
        part[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t w = 0; w < wave; ++w)
        before += part[w];
    if (i < A.nrows)
        A.counts[i] = before + incl - count;
    if (threadIdx.x == 0u && i < A.nrows)
        A.groups[i / kSurfGroup] = part[0] + part[1] + part[2] + part[3];
}

// the exclusive scan of the group totals in place: thread i owns a contiguous share of the groups
__global__ __launch_bounds__(256) void k_surf_groups(const SurfArgs A)
{
    __shared__ uint32_t share[256];
    const uint32_t per = (A.ngroups + 255u) / 256u, a = threadIdx.x * per < A.ngroups ? threadIdx.x * per : A.ngroups;
    const uint32_t b = a + per < A.ngroups ? a + per : A.ngroups;
    uint32_t sum = 0u;
    for (uint32_t g = a; g < b; ++g)
        sum += A.groups[g];
    share[threadIdx.x] = sum;
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t i = 0; i < threadIdx.x; ++i)
        before += share[i];
    for (uint32_t g = a; g < b; ++g) {
        const uint32_t n = A.groups[g];
        A.groups[g] = before;
        before += n;
    }
    if (threadIdx.x == 255u) {  // `before` is the grand total; the count passes' atomics are complete
        uint32_t faces = 0u;
        for (uint32_t d = 0; d < 6u; ++d)
            faces += A.summary[kSurfSumFacesDir + d];
        A.summary[kSurfSumFaces] = faces;
        A.summary[kSurfSumQuads] = before;
        A.summary[kSurfSumWritten] = before < A.capacity ? before : A.capacity;
    }
}

__global__ __launch_bounds__(256) void k_surf_emit_yz(const SurfArgs A)
{
    const uint32_t j = (uint32_t)flat_block() * 256u + threadIdx.x;
    if (j >= A.nryz)
        return;
    const uint32_t pos = surf_row_start(A, A.nrx + j);
    SurfTally t{};
    uint32_t dir;
    if (pos < A.capacity)
        surf_row_yz<true>(A, j, pos, t, dir);
}

__global__ __launch_bounds__(256) void k_surf_emit_x(const SurfArgs A, uint32_t x64)
{
    const uint32_t i = (uint32_t)flat_block() * 256u + threadIdx.x;
    const uint32_t x = i % x64, q = i / x64, z = q % (uint32_t)A.d[2], d = q / (uint32_t)A.d[2];
    if (d >= 2u || x >= (uint32_t)A.d[0])
        return;
    const uint32_t pos = surf_row_start(A, surf_row_index_x(A, d, (int32_t)x, (int32_t)z));
    SurfTally t{};
    if (pos < A.capacity)
        surf_row_x<true>(A, d, (int32_t)x, (int32_t)z, pos, t);
}

// host entry point (vxrt_api.hip): arguments validated there (surf_layout accepts them).  Asynchronous on `stream`.
hipError_t extract_surface(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t mode, void* work, vxrt_quad* quads,
                           uint32_t capacity, int32_t* verts, uint32_t* tris, vxrt_surface_summary* summary, hipStream_t stream)
{
    SurfLayout L;
    if (!surf_layout(o, d, L))
        return hipErrorInvalidValue;
    SurfArgs A{};
    surf_args(A, L, d, mode, work, (uint32_t*)quads, capacity, verts, tris, (uint32_t*)summary);
    hipError_t e;
    if ((e = hipMemsetAsync(summary, 0, sizeof(vxrt_surface_summary), stream)) != hipSuccess)
        return e;
    if ((e = read_region(W, L.ho, L.hd, (uint32_t*)((char*)work + L.halo), stream)) != hipSuccess)
        return e;
    const uint32_t x64 = ((uint32_t)d[0] + 63u) / 64u * 64u;
    const dim3 gyz = grid_2d((L.nryz + 255u) / 256u), gx = grid_2d((2u * (uint64_t)d[2] * x64 + 255u) / 256u);
    hipLaunchKernelGGL(k_surf_count_yz, gyz, dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_surf_count_x, gx, dim3(256), 0, stream, A, x64);
    hipLaunchKernelGGL(k_surf_scan, grid_2d(L.ngroups), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_surf_groups, dim3(1), dim3(256), 0, stream, A);
    if (A.capacity) {
        hipLaunchKernelGGL(k_surf_emit_x, gx, dim3(256), 0, stream, A, x64);
        hipLaunchKernelGGL(k_surf_emit_yz, gyz, dim3(256), 0, stream, A);
    }
    return hipGetLastError();
}

}  // namespace vxrt
