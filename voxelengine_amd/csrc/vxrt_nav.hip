// vxrt_nav.hip -- navigation fields over a box of the resident brickmap (include/vxrt.h, vxrt_nav_field / vxrt_nav_paths;
// host side in vxrt_api.hip, the shared logic in vxrt_nav.hpp).  A field is these launches on the caller's stream:
//
//   k_read_region   (vxrt_region.hip, unchanged) the halo's bits into the workspace.
//   k_nav_xpass     one lane per word of a halo row: the AND of the W empty bits x .. x + W - 1 (funnel shifts across
//                   word borders), and their OR for the rows below B's cells (the footprint's support).
//   k_nav_ypass     one lane per word: the AND over the agent's H rows.
//   k_nav_zpass     one lane per word of B (grid-stride): the AND over W rows in z (free), the support OR, walkable = free
//                   and supported cut to B; the node count summed per workgroup.
//   k_nav_goals     one lane per goal: a node joins level 0 and lists the tiles around it.
//   k_nav_level     one launch per BFS level: one 256-lane workgroup per listed tile (32 x 16 x 16 cells, one region word
//                   per lane), grid-stride over the level's list.  Each word pulls its new cells from the frontier
//                   (vxrt_nav.hpp); the tile's bounding box of new cells, reduced in LDS, lists the tiles that can hold
//                   their predecessors for the next level.  The host reads the next list's length every kNavSyncLevels
//                   levels and stops when it is 0: no grid-wide barrier, no workgroup waits for another.
//   k_nav_next      one lane per cell: the first valid move to dist - 1, from dist alone.
//   k_nav_finish    one lane: levels and tiles_total.
#include "../../include/vxrt.h"
#include "vxrt_nav.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_nav_agent) == 16, "nav agent layout");
static_assert(sizeof(vxrt_nav_summary) == 32, "nav summary layout");

constexpr uint32_t kNavSyncLevels = 16;  // levels launched between two reads of the termination flag
constexpr uint32_t kNavLevelGroups = 512;

// i = x + a (y + b z): 32-bit divisions when i fits (always but for halo boxes of more than 2^32 words)
__device__ inline void nav_split(uint64_t i, uint32_t a, uint32_t b, uint32_t& x, uint32_t& y, uint32_t& z)
{
    if (i >> 32) {
        const uint64_t r = i / a;
        x = (uint32_t)(i % a);
        y = (uint32_t)(r % b);
        z = (uint32_t)(r / b);
    } else {
        const uint32_t j = (uint32_t)i, r = j / a;
        x = j % a;
        y = r % b;
        z = r / b;
    }
}

__global__ __launch_bounds__(256) void k_nav_xpass(const NavArgs A, uint64_t n)
{
    const uint64_t i = flat_thread();
    if (i >= n)
        return;
    uint32_t xw, y, z;
    nav_split(i, A.wb, A.hy, xw, y, z);
    nav_xpass_word(A, xw, y, z);
}

__global__ __launch_bounds__(256) void k_nav_ypass(const NavArgs A, uint64_t n)
{
    const uint64_t i = flat_thread();
    if (i >= n)
        return;
    uint32_t xw, y, z;
    nav_split(i, A.wb, (uint32_t)A.d[1], xw, y, z);
    nav_ypass_word(A, xw, y, z);
}

// grid-stride over at most kNavZpassGroups workgroups: one node-count atomic per workgroup (one per wave serialises on
// the single counter: 65k waves of a 1024 x 128 x 1024 box took 0.65 ms)
constexpr uint32_t kNavZpassGroups = 2048;

__global__ __launch_bounds__(256) void k_nav_zpass(const NavArgs A)
{
    __shared__ uint32_t part[4];
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < A.nb; i += (uint64_t)gridDim.x * 256u) {
        uint32_t xw, y, z;
        nav_split(i, A.wb, (uint32_t)A.d[1], xw, y, z);
        c += nav_zpass_word(A, xw, y, z);
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63u) == 0)
        part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0 && part[0] + part[1] + part[2] + part[3])
        atomicAdd(A.summary + kNavSumNodes, part[0] + part[1] + part[2] + part[3]);
}

__global__ __launch_bounds__(256) void k_nav_goals(const NavArgs A)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= A.ngoals)
        return;
    const int r = nav_goal(A, g);
    atomicAdd(A.summary + (r ? kNavSumGoalsUsed : kNavSumGoalsIgnored), 1u);
    if (r == 2)
        atomicAdd(A.summary + kNavSumReached, 1u);
}

__global__ __launch_bounds__(256) void k_nav_level(const NavArgs A, uint32_t lv)
{
    __shared__ int32_t box[6];  // y lo, y hi, z lo, z hi, any bit 0, any bit 31
    __shared__ uint32_t found;
    const uint32_t slot = lv % kNavSlots;
    const uint32_t count = A.ctrl[slot];  // written by the launches before this one
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.ctrl[(lv + 2u) % kNavSlots] = 0u;  // read by level lv - 1 (done), appended to by level lv + 1
        if (count)
            A.summary[kNavSumVisits] += count;
    }
    const uint32_t lane = threadIdx.x, ly = lane & (kNavTileY - 1), lz = lane / kNavTileY;
    for (uint32_t k = blockIdx.x; k < count; k += gridDim.x) {
        const uint32_t t = A.list[(uint64_t)slot * A.ntiles + k];
        const uint32_t tx = t % A.wb, tr = t / A.wb, ty = tr % A.nty, tz = tr / A.nty;
        if (lane == 0) {
            box[0] = box[2] = 0x7FFFFFFF;
            box[1] = box[3] = -1;
            box[4] = box[5] = 0;
            found = 0u;
        }
        __syncthreads();
        const uint32_t y = ty * kNavTileY + ly, z = tz * kNavTileZ + lz;
        uint32_t nw = 0;
        if (y < (uint32_t)A.d[1] && z < (uint32_t)A.d[2])
            nw = nav_level_word(A, lv, tx, y, z);
        if (nw) {
            atomicMin(&box[0], (int32_t)y);
            atomicMax(&box[1], (int32_t)y);
            atomicMin(&box[2], (int32_t)z);
            atomicMax(&box[3], (int32_t)z);
            if (nw & 1u)
                box[4] = 1;
            if (nw >> 31)
                box[5] = 1;
            atomicAdd(&found, (uint32_t)__popc(nw));
        }
        __syncthreads();
        if (lane == 0) {
            A.stamp[(uint64_t)((lv + 1u) & 1u) * A.ntiles + t] = lv + 1u;
            if (found) {
                atomicAdd(A.summary + kNavSumReached, found);
                atomicMax(A.summary + kNavSumMaxDist, lv + 1u);
                nav_mark_around(A, lv + 1u, tx, box[4] != 0, box[5] != 0, box[0], box[1], box[2], box[3]);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_nav_next(const NavArgs A)
{
    const uint64_t i = flat_thread();
    if (i >= A.nvox)
        return;
    uint32_t x, y, z;
    nav_split(i, (uint32_t)A.d[0], (uint32_t)A.d[1], x, y, z);
    A.next[i] = nav_next_cell(A, x, y, z);
}

__global__ void k_nav_finish(const NavArgs A)
{
    A.summary[kNavSumLevels] = A.summary[kNavSumGoalsUsed] ? A.summary[kNavSumMaxDist] + 1u : 0u;
    A.summary[kNavSumTiles] = A.ntiles;
}

__global__ __launch_bounds__(256) void k_nav_paths(const NavPathArgs P)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < P.n; i += (uint64_t)gridDim.x * 256u)
        nav_path(P, i);
}

// host entry point (vxrt_api.hip): arguments validated there.  Returns when the field is complete (the stream is
// synchronised every kNavSyncLevels levels).
hipError_t nav_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], const vxrt_nav_agent& ag, const int32_t* goals,
                     uint32_t ngoals, uint32_t max_dist, void* work, uint32_t* walkable, uint8_t* next, uint32_t* dist,
                     vxrt_nav_summary* summary, hipStream_t stream)
{
    NavLayout L;
    if (!nav_layout(d, ag.width, ag.height, ag.climb, ag.drop, L))
        return hipErrorInvalidValue;
    NavArgs A{};
    nav_args(A, L, o, d, ag.width, ag.height, ag.climb, ag.drop, goals, ngoals, work, walkable, next, dist, (uint32_t*)summary);
    hipError_t e;
    if ((e = hipMemsetAsync(summary, 0, sizeof(vxrt_nav_summary), stream)) != hipSuccess ||
        (e = hipMemsetAsync(A.ctrl, 0, kNavCtrlWords * 4u, stream)) != hipSuccess ||
        (e = hipMemsetAsync(A.mark, 0, (size_t)L.ntiles * 4u, stream)) != hipSuccess ||
        (e = hipMemsetAsync(A.stamp, 0xFF, (size_t)L.ntiles * 8u, stream)) != hipSuccess ||
        (e = hipMemsetAsync(A.vis, 0, (size_t)L.nb * 4u, stream)) != hipSuccess ||
        (e = hipMemsetAsync(A.front[0], 0, (size_t)L.nb * 4u, stream)) != hipSuccess ||
        (e = hipMemsetAsync(A.dist, 0xFF, (size_t)L.nvox * 4u, stream)) != hipSuccess)
        return e;
    // the halo box; one that int32 cannot hold lies wholly outside the world (|origin| > 2^31 - 2^28 - 40), so it is empty
    const int64_t hlo = (int64_t)o[1] - 1, hhi[3] = {(int64_t)o[0] + d[0] + ag.width - 1, (int64_t)o[1] + d[1] + ag.height - 1,
                                                    (int64_t)o[2] + d[2] + ag.width - 1};
    if (hlo < INT32_MIN || hhi[0] > INT32_MAX || hhi[1] > INT32_MAX || hhi[2] > INT32_MAX) {
        if ((e = hipMemsetAsync((uint32_t*)work + L.halo, 0, (size_t)L.wh * L.hy * L.hz * 4u, stream)) != hipSuccess)
            return e;
    } else {
        const int32_t ho[3] = {o[0], (int32_t)hlo, o[2]};
        const int32_t hd[3] = {d[0] + ag.width - 1, (int32_t)L.hy, (int32_t)L.hz};
        if ((e = read_region(W, ho, hd, (uint32_t*)work + L.halo, stream)) != hipSuccess)
            return e;
    }
    const uint64_t nx = (uint64_t)L.wb * L.hy * L.hz, ny = (uint64_t)L.wb * (uint64_t)d[1] * L.hz;
    hipLaunchKernelGGL(k_nav_xpass, grid_2d((nx + 255u) / 256u), dim3(256), 0, stream, A, nx);
    hipLaunchKernelGGL(k_nav_ypass, grid_2d((ny + 255u) / 256u), dim3(256), 0, stream, A, ny);
    const uint64_t zb = (L.nb + 255u) / 256u;
    hipLaunchKernelGGL(k_nav_zpass, dim3(zb < kNavZpassGroups ? (unsigned)zb : kNavZpassGroups), dim3(256), 0, stream, A);
    if (ngoals)
        hipLaunchKernelGGL(k_nav_goals, dim3((ngoals + 255u) / 256u), dim3(256), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    const unsigned groups = L.ntiles < kNavLevelGroups ? L.ntiles : kNavLevelGroups;
    for (uint32_t lv = 0; ngoals && lv < max_dist;) {
        const uint32_t batch = max_dist - lv < kNavSyncLevels ? max_dist - lv : kNavSyncLevels;
        for (uint32_t k = 0; k < batch; ++k, ++lv)
            hipLaunchKernelGGL(k_nav_level, dim3(groups), dim3(256), 0, stream, A, lv);
        uint32_t pending = 0;
        if ((e = hipMemcpyAsync(&pending, A.ctrl + lv % kNavSlots, 4u, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
            (e = hipStreamSynchronize(stream)) != hipSuccess)
            return e;
        if (!pending)
            break;
    }
    hipLaunchKernelGGL(k_nav_next, grid_2d(((uint64_t)L.nvox + 255u) / 256u), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_nav_finish, dim3(1), dim3(1), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess)
        return e;
    return hipStreamSynchronize(stream);
}

hipError_t nav_paths(const NavPathArgs& P, hipStream_t stream)
{
    const uint64_t blocks = (P.n + 255u) / 256u;
    hipLaunchKernelGGL(k_nav_paths, dim3(blocks > 4096u ? 4096u : (unsigned)blocks), dim3(256), 0, stream, P);
    return hipGetLastError();
}

}  // namespace vxrt
