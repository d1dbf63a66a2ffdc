// vxrt_islands.hip -- floating-island detection in a box of the resident brickmap (include/vxrt.h, vxrt_find_islands; host
// side in vxrt_api.hip, the shared logic in vxrt_islands.hpp).  One call is eight launches on the caller's stream:
//
//   k_read_region      (vxrt_region.hip, unchanged) the box's bits into the workspace.
//   k_isl_local        one 256-lane workgroup per 32 x 16 x 16 tile, one region word per lane: LDS parents start at the
//                      voxel's run start along x (ctz / clz of the masked row word), then one LDS union per run of face
//                      pairs in y and z, then the tile-local roots written to the global parents, lane = x (coalesced).
//   k_isl_merge        one lane per region word: the unions across tile borders (x: every word border; y, z: the first
//                      row of a tile), one per run of face pairs, on global parents.  The work scales with the tiles'
//                      surface, not their volume.
//   k_isl_flatten      one lane per voxel index: parent = root = component id - 1, the label, the root bits by ballot,
//                      one atomicOr per (wave, root) for anchor voxels, the component count.
//   k_isl_scan_blocks  one workgroup per 1024 root words: island roots = roots & ~anchored, the in-block prefix.
//   k_isl_scan_top     one workgroup: the block prefix and the island count.
//   k_isl_rows         one lane per root word: the table rows of its island roots (id, empty box) in ascending id.
//   k_isl_output       one wave per 16 pairs of region words, one lane per voxel: the floating words by ballot, the
//                      island voxel count, and per-island voxel counts and boxes accumulated in the wave across its
//                      pairs and flushed with one set of atomics when the island changes (not one per voxel).
// Every root is the minimum index of its component (vxrt_islands.hpp), so all outputs are scheduling-independent.
#include "../../include/vxrt.h"
#include "vxrt_islands.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_island) == 32, "island row layout");
static_assert(sizeof(vxrt_island_summary) == 12, "island summary layout");

__global__ __launch_bounds__(256) void k_isl_local(const IslandsArgs A, uint32_t ntiles, uint32_t ntx, uint32_t nty)
{
    __shared__ uint32_t lp[kIslTileVoxels];
    __shared__ uint32_t rows[kIslTileRows];
    const uint32_t b = (uint32_t)flat_block();
    if (b >= ntiles)
        return;
    const uint32_t tx = b % ntx, t = b / ntx, ty = t % nty, tz = t / nty;
    const uint32_t lane = threadIdx.x;
    rows[lane] = isl_tile_row(A, tx, ty, tz, lane);
    __syncthreads();
    // lane = x over 8 rows per step: LDS without bank conflicts, global writes coalesced
    const uint32_t x = lane & 31u, r0 = lane >> 5;
    for (uint32_t r = r0; r < kIslTileRows; r += 8u)
        isl_tile_init_voxel(lp, rows[r], x, r);
    __syncthreads();
    isl_tile_union_row(lp, rows, lane);
    __syncthreads();
    for (uint32_t r = r0; r < kIslTileRows; r += 8u) {
        uint32_t g, val;
        if (isl_tile_parent(A, lp, rows, tx, ty, tz, x, r, g, val))
            A.parent[g] = val;
    }
}

__global__ __launch_bounds__(256) void k_isl_merge(const IslandsArgs A)
{
    const uint64_t wi = flat_thread();
    if (wi >= A.nbits)
        return;
    const uint32_t xw = (uint32_t)(wi % A.wpr), row = (uint32_t)(wi / A.wpr);
    isl_merge_word(A, xw, row % (uint32_t)A.d[1], row / (uint32_t)A.d[1]);
}

// one wave per 64 consecutive voxel indices per step (grid-stride): the root words are the waves' ballots
__global__ __launch_bounds__(256) void k_isl_flatten(const IslandsArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * 4u;
    uint32_t comps = 0;
    for (uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6); q < A.nwords / 2u; q += nwaves) {
        const uint32_t i = 64u * q + lane;
        uint32_t root = 0;
        bool anchor = false, solid = false;
        if (i < A.nvox)
            solid = isl_flatten_voxel(A, i, root, anchor);
        const unsigned long long m = __ballot(solid && root == i);
        if (lane == 0)
            A.roots[2u * q] = (uint32_t)m;
        else if (lane == 32)
            A.roots[2u * q + 1u] = (uint32_t)(m >> 32);
        comps += (uint32_t)__popcll(m);
        // anchor voxels: one atomicOr per distinct root in the wave
        bool want = solid && anchor;
        for (unsigned long long p = __ballot(want); p; p = __ballot(want)) {
            const int leader = __ffsll((long long)p) - 1;
            const uint32_t r = (uint32_t)__shfl((int)root, leader, 64);
            if ((int)lane == leader)
                isl_mark_anchor(A, r);
            if (want && root == r)
                want = false;
        }
    }
    if (lane == 0 && comps)
        atomicAdd(A.summary + 0, comps);
}

// exclusive scan of one value per lane of a 256-lane workgroup; returns the workgroup's total in *total
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* sh, uint32_t& total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t s = 1; s < 256u; s <<= 1) {
        const uint32_t a = t >= s ? sh[t - s] : 0u;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    total = sh[255];
    const uint32_t ex = sh[t] - v;
    __syncthreads();
    return ex;
}

__global__ __launch_bounds__(256) void k_isl_scan_blocks(const IslandsArgs A)
{
    __shared__ uint32_t sh[256];
    const uint32_t b = blockIdx.x, w0 = b * kIslScanBlock + 4u * threadIdx.x;
    uint32_t iw[4], c[4], s = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t w = w0 + (uint32_t)k;
        iw[k] = w < A.nwords ? isl_island_word(A, w) : 0u;
        c[k] = (uint32_t)__popc(iw[k]);
        s += c[k];
    }
    uint32_t total;
    uint32_t ex = block_exclusive_scan(s, sh, total);
    for (int k = 0; k < 4; ++k) {
        const uint32_t w = w0 + (uint32_t)k;
        if (w < A.nwords) {
            A.roots[w] = iw[k];
            A.prefix[w] = ex;
        }
        ex += c[k];
    }
    if (threadIdx.x == 0)
        A.blocks[b] = total;
}

__global__ __launch_bounds__(256) void k_isl_scan_top(const IslandsArgs A)
{
    __shared__ uint32_t sh[256];
    const uint32_t per = (A.nblocks + 255u) / 256u, b0 = threadIdx.x * per;
    uint32_t s = 0;
    for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < A.nblocks)
            s += A.blocks[b0 + k];
    uint32_t total;
    uint32_t ex = block_exclusive_scan(s, sh, total);
    for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < A.nblocks) {
            const uint32_t v = A.blocks[b0 + k];
            A.blocks[b0 + k] = ex;
            ex += v;
        }
    if (threadIdx.x == 0)
        A.summary[1] = total;
}

__global__ __launch_bounds__(256) void k_isl_rows(const IslandsArgs A)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= A.nwords)
        return;
    uint32_t iw = A.roots[w];
    uint32_t rank = A.blocks[w / kIslScanBlock] + A.prefix[w];
    for (; iw && rank < A.max_islands; iw &= iw - 1u, ++rank)
        isl_init_row(A, rank, 32u * w + (uint32_t)__builtin_ctz(iw));
}

constexpr uint32_t kIslPairsPerWave = 16;

__global__ __launch_bounds__(256) void k_isl_output(const IslandsArgs A, uint32_t nchunks)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t npairs = (A.nbits + 1u) / 2u;
    uint32_t voxels = 0;
    // the island whose counts the wave holds (wave-uniform), and this lane's share of them
    uint32_t cur = 0xFFFFFFFFu, pc = 0;
    int32_t plo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, phi[3] = {(int32_t)0x80000000, (int32_t)0x80000000, (int32_t)0x80000000};
    auto flush = [&]() {
        const uint32_t n = wave_sum(pc);
        int32_t lo[3], hi[3];
        for (int k = 0; k < 3; ++k) {
            lo[k] = wave_min(plo[k]);
            hi[k] = wave_max(phi[k]);
            plo[k] = 0x7FFFFFFF;
            phi[k] = (int32_t)0x80000000;
        }
        if (lane == 0)
            isl_add_to_row(A, cur, n, lo, hi);
        pc = 0;
    };
    for (uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6); c < nchunks; c += gridDim.x * 4u) {
        for (uint32_t j = 0; j < kIslPairsPerWave; ++j) {
            const uint64_t p = (uint64_t)c * kIslPairsPerWave + j;
            if (p >= npairs)
                break;
            const uint64_t wi = 2u * p + (lane >> 5);
            uint32_t rank = 0xFFFFFFFFu, wx = 0, wy = 0, wz = 0;
            bool isl = false;
            if (wi < A.nbits) {
                const uint32_t xw = (uint32_t)(wi % A.wpr), row = (uint32_t)(wi / A.wpr);
                wx = 32u * xw + (lane & 31u);
                wy = row % (uint32_t)A.d[1];
                wz = row / (uint32_t)A.d[1];
                if (wx < (uint32_t)A.d[0])
                    isl = isl_voxel_island(A, A.bits[wi], wx, wy, wz, rank);
            }
            const unsigned long long m = __ballot(isl);
            if (lane == 0 && 2u * p < A.nbits)
                A.floating[2u * p] = (uint32_t)m;
            else if (lane == 32 && wi < A.nbits)
                A.floating[wi] = (uint32_t)(m >> 32);
            voxels += isl ? 1u : 0u;
            if (!A.table)
                continue;
            const int32_t g[3] = {A.o[0] + (int32_t)wx, A.o[1] + (int32_t)wy, A.o[2] + (int32_t)wz};
            for (;;) {
                const unsigned long long pend = __ballot(rank != 0xFFFFFFFFu);
                if (!pend)
                    break;
                if (!__ballot(rank != 0xFFFFFFFFu && rank == cur)) {
                    if (cur != 0xFFFFFFFFu)
                        flush();
                    cur = (uint32_t)__shfl((int)rank, __ffsll((long long)pend) - 1, 64);
                }
                if (rank != 0xFFFFFFFFu && rank == cur) {
                    ++pc;
                    for (int k = 0; k < 3; ++k) {
                        plo[k] = min(plo[k], g[k]);
                        phi[k] = max(phi[k], g[k]);
                    }
                    rank = 0xFFFFFFFFu;
                }
            }
        }
    }
    if (A.table && cur != 0xFFFFFFFFu)
        flush();
    const uint32_t n = wave_sum(voxels);
    if (lane == 0 && n)
        atomicAdd(A.summary + 2, n);
}

// host entry point (vxrt_api.hip): arguments validated there
hipError_t find_islands(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t anchors, void* work,
                        uint32_t* floating, uint32_t* labels, vxrt_island* table, uint32_t max_islands,
                        vxrt_island_summary* summary, hipStream_t stream)
{
    IslandsLayout L;
    if (!islands_layout(d, L))
        return hipErrorInvalidValue;
    IslandsArgs A{};
    islands_args(A, L, o, d, anchors, work, floating, labels, (int32_t*)table, max_islands, (uint32_t*)summary);
    hipError_t e;
    if ((e = hipMemsetAsync(A.anchor, 0, (size_t)L.nwords * 4u, stream)) != hipSuccess)
        return e;
    if ((e = hipMemsetAsync(summary, 0, sizeof(vxrt_island_summary), stream)) != hipSuccess)
        return e;
    if ((e = read_region(W, o, d, (uint32_t*)work + L.bits, stream)) != hipSuccess)
        return e;
    const uint32_t ntx = L.wpr, nty = ((uint32_t)d[1] + kIslTileY - 1) / kIslTileY, ntz = ((uint32_t)d[2] + kIslTileZ - 1) / kIslTileZ;
    const uint64_t ntiles = (uint64_t)ntx * nty * ntz;  // <= 2^28
    hipLaunchKernelGGL(k_isl_local, grid_2d(ntiles), dim3(256), 0, stream, A, (uint32_t)ntiles, ntx, nty);
    hipLaunchKernelGGL(k_isl_merge, grid_2d((L.nbits + 255u) / 256u), dim3(256), 0, stream, A);
    const uint32_t fw = (L.nwords / 2u + 3u) / 4u;
    hipLaunchKernelGGL(k_isl_flatten, dim3(fw > 65536u ? 65536u : fw), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_isl_scan_blocks, dim3(L.nblocks), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_isl_scan_top, dim3(1), dim3(256), 0, stream, A);
    if (A.table)
        hipLaunchKernelGGL(k_isl_rows, dim3((L.nwords + 255u) / 256u), dim3(256), 0, stream, A);
    const uint64_t npairs = (L.nbits + 1u) / 2u;
    const uint32_t nchunks = (uint32_t)((npairs + kIslPairsPerWave - 1) / kIslPairsPerWave);
    const uint32_t ob = (nchunks + 3u) / 4u;
    hipLaunchKernelGGL(k_isl_output, dim3(ob > 65536u ? 65536u : (ob ? ob : 1u)), dim3(256), 0, stream, A, nchunks);
    return hipGetLastError();
}

}  // namespace vxrt
