// vxrt_voxelize.hip -- a triangle mesh into region-layout bits (include/vxrt.h, vxrt_voxelize_mesh; host side in
// vxrt_api.hip, the shared logic in vxrt_voxelize.hpp).  A call reads no world.  It is these operations on the caller's
// stream:
//
//   memsets         the output bits, the summary, the counters and (solid) the toggle field.
//   k_vox_setup     one lane per triangle: validity, the clipped voxel boxes, the item count; a scan over the workgroup's
//                   256 counts gives every triangle its start within the group and the group its total; the summary's
//                   triangle counters.
//   k_vox_groups    one workgroup: the exclusive scan of the group totals (uint64) and the grand total.
//   k_vox_work      persistent waves take items from a ticket counter (one atomic per wave and item, as queue_take of the
//                   render kernels) until it passes the total.  The triangle of an item is found by two binary searches;
//                   its constants are recomputed from the vertices, wave-uniform.  A surface item culls 64 blocks, then the
//                   64 rows of each surviving block, then writes a row's 64 voxels with at most two atomic ORs; a solid
//                   item XORs one toggle bit per covered column.
//   k_vox_final     one lane per output word, the words of 64 / wpr whole rows per wave: the parities of a row's toggle
//                   words by one ballot, the suffix XOR, the OR with the surface bits, the popcounts.
#include "../../include/vxrt.h"
#include "vxrt_voxelize.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_voxelize_summary) == 32, "voxelize summary layout");
static_assert(kVoxMaxDim / 32 <= 32, "a row's words fit half a wave");

struct VoxWave {
    uint32_t lane;
    template <class F>
    __device__ uint64_t ballot(F f) const { return __ballot(f(lane)); }
    __device__ bool first() const { return lane == 0u; }
};

__global__ __launch_bounds__(256) void k_vox_setup(const VoxArgs A)
{
    __shared__ uint32_t part[4];
    const uint32_t t = blockIdx.x * kVoxGroup + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t flags = 0u, count = 0u;
    if (t < A.nt)
        count = vox_setup_lane(A, t, flags);
    // inclusive scan of the counts over the wave, then over the workgroup's four waves
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
    if (t < A.nt)
        vox_setup_store(A, t, before + incl - count);
    if (threadIdx.x == 0)
        A.group_prefix[blockIdx.x] = (uint64_t)part[0] + part[1] + part[2] + part[3];
    const uint32_t inv = wave_sum(flags & kVoxInvalid ? 1u : 0u), deg = wave_sum(flags & kVoxDegenerate ? 1u : 0u);
    const uint32_t out = wave_sum(flags & kVoxOutside ? 1u : 0u);
    if (lane == 0u) {
        if (inv)
            atomicAdd(A.summary + kVoxSumInvalid, inv);
        if (deg)
            atomicAdd(A.summary + kVoxSumDegenerate, deg);
        if (out)
            atomicAdd(A.summary + kVoxSumOutside, out);
    }
}

// the exclusive scan of the group totals in place: thread i owns a contiguous share of the groups
__global__ __launch_bounds__(256) void k_vox_groups(const VoxArgs A)
{
    __shared__ uint64_t share[256];
    const uint32_t per = (A.ngroups + 255u) / 256u, a = threadIdx.x * per, b = a + per < A.ngroups ? a + per : A.ngroups;
    uint64_t sum = 0;
    for (uint32_t g = a; g < b; ++g)
        sum += A.group_prefix[g];
    share[threadIdx.x] = sum;
    __syncthreads();
    uint64_t before = 0;
    for (uint32_t i = 0; i < threadIdx.x; ++i)
        before += share[i];
    for (uint32_t g = a; g < b; ++g) {
        const uint64_t n = A.group_prefix[g];
        A.group_prefix[g] = before;
        before += n;
    }
    if (threadIdx.x == 255u)
        A.counters[kVoxTotal] = before;
    if (threadIdx.x == 0u)
        A.summary[kVoxSumTriangles] = A.nt;
}

__global__ __launch_bounds__(256) void k_vox_work(const VoxArgs A)
{
    const VoxWave wave{threadIdx.x & 63u};
    const uint64_t total = A.counters[kVoxTotal];
    for (;;) {
        unsigned long long item = 0;
        if (wave.lane == 0u)
            item = atomicAdd((unsigned long long*)(A.counters + kVoxTicket), 1ull);
        item = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(item >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)item);
        if (item >= total)
            return;
        uint32_t t, q;
        vox_find(A, item, t, q);
        VoxTri T;
        vox_tri_load(A, t, T);
        uint32_t ns, nd;
        vox_items(A, T, ns, nd);
        if (q < ns) {
            VoxSat S;
            vox_sat_setup(T, S);
            vox_surface_item(A, T, S, q, wave);
        } else {
            VoxSolid S;
            vox_solid_setup(T, S);
            vox_solid_lane(A, T, S, q - ns, wave.lane);
        }
    }
}

__global__ __launch_bounds__(256) void k_vox_final(const VoxArgs A, uint64_t nrows)
{
    const uint32_t lane = threadIdx.x & 63u, rpw = 64u / A.wpr;  // whole rows per wave, 2 or more
    const uint64_t w = flat_block() * 4u + (threadIdx.x >> 6);
    const uint32_t r = lane / A.wpr, idx = lane - r * A.wpr;
    const uint64_t row = w * rpw + r;
    const bool live = r < rpw && row < nrows;
    const uint64_t g = row * A.wpr + idx;
    const uint64_t odd = __ballot(live && vox_final_parity(A, g));
    VoxTally t{};
    if (live) {
        // the lanes lane + 1 .. lane + wpr - 1 - idx hold the higher words of this row
        const uint64_t above = (odd >> lane >> 1) & ((1ull << (A.wpr - 1u - idx)) - 1ull);
        vox_final_word(A, g, (__popcll(above) & 1) != 0, t);
    }
    t.set = wave_sum(t.set);
    t.surface = wave_sum(t.surface);
    t.solid = wave_sum(t.solid);
    if (lane == 0u) {
        if (t.set)
            atomicAdd(A.summary + kVoxSumSet, t.set);
        if (t.surface)
            atomicAdd(A.summary + kVoxSumSurface, t.surface);
        if (t.solid)
            atomicAdd(A.summary + kVoxSumSolid, t.solid);
    }
}

// host entry point (vxrt_api.hip): arguments validated there (vox_layout accepts them).  Asynchronous on `stream`.
hipError_t voxelize_mesh(const int32_t* verts, uint32_t nv, const uint32_t* tris, uint32_t nt, const int32_t d[3], uint32_t modes,
                         void* work, uint32_t* bits, vxrt_voxelize_summary* summary, uint32_t work_waves, hipStream_t stream)
{
    VoxLayout L;
    if (!vox_layout(d, nt, L))
        return hipErrorInvalidValue;
    VoxArgs A{};
    vox_args(A, L, verts, nv, tris, nt, d, modes, work, bits, (uint32_t*)summary);
    hipError_t e;
    if ((e = hipMemsetAsync(bits, 0, L.words * 4u, stream)) != hipSuccess)
        return e;
    if ((e = hipMemsetAsync(summary, 0, sizeof(vxrt_voxelize_summary), stream)) != hipSuccess)
        return e;
    if (nt == 0)
        return hipSuccess;
    if ((e = hipMemsetAsync(A.counters, 0, 256u, stream)) != hipSuccess)
        return e;
    if ((modes & kVoxSolid) && (e = hipMemsetAsync(A.toggle, 0, L.words * 4u, stream)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_vox_setup, dim3(L.ngroups), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_vox_groups, dim3(1), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_vox_work, dim3((work_waves + 3u) / 4u), dim3(256), 0, stream, A);
    const uint64_t nrows = (uint64_t)d[1] * (uint64_t)d[2], nwaves = (nrows + 64u / L.wpr - 1u) / (64u / L.wpr);
    hipLaunchKernelGGL(k_vox_final, grid_2d((nwaves + 3u) / 4u), dim3(256), 0, stream, A, nrows);
    return hipGetLastError();
}

}  // namespace vxrt
