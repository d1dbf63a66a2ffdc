// vxrt_edit.hip -- voxel editing of the resident brickmap (include/vxrt.h, vxrt_edit_voxels; host side in vxrt_api.hip).
//
// Two launches per edit call, around one host step:
//   k_edit_bricks  one 256-thread workgroup per touched brick cell (the cells in the union of the ops' clipped brick boxes,
//                  HBM cell order), in the structure of k_fill_bricks: the old image into LDS, the ops that meet the brick
//                  filtered into LDS in order (from the last op that covers the whole brick: earlier ones cannot matter
//                  there), one voxel per lane evaluated against them (last match wins), packed by __ballot, extents reduced
//                  through LDS.  Writes the image, the packed extents and {old slot, non-empty | changed << 1} to scratch:
//                  nothing in the world tables.
//   (host)         reads the flags back, frees and assigns slots (vxrt_edit.hpp, edit_plan_slots), grows the pool if needed.
//   k_edit_commit  per changed cell: the image to its slot (16 B per lane), the cell record, the coarse bit (word
//                  atomicOr / atomicAnd: up to 32 cells share a word); per freed slot that stays free: zeros.
#include "../../include/vxrt.h"
#include "vxrt_edit.hpp"
#include "vxrt_kernels.hpp"
#include "vxrt_region.hpp"

namespace vxrt {

static_assert(sizeof(EditOpDev) == 56, "edit op layout (the host copies it as bytes)");

__global__ __launch_bounds__(256) void k_edit_bricks(const uint32_t* __restrict__ cells, uint32_t n,
                                                     const EditOpDev* __restrict__ ops, uint32_t nops,
                                                     const uint2* __restrict__ meta, const uint4* __restrict__ pool,
                                                     uint4* __restrict__ scratch, uint32_t* __restrict__ ext,
                                                     uint2* __restrict__ info, int f, int cx, int cz)
{
    __shared__ uint4 old_vecs[256];  // the old image, f <= 32: 4 KiB
    __shared__ uint16_t list[kEditMaxOps];
    __shared__ uint8_t meets[kEditMaxOps];
    __shared__ int red[8];  // min xyz, max xyz, any, changed
    __shared__ int first, count;
    const uint32_t i = blockIdx.x + blockIdx.y * gridDim.x;  // 2-D grid: more cells than one grid axis holds
    if (i >= n)
        return;
    const uint32_t cell = cells[i];
    int bx, by, bz;
    hbm_cell(cell, cx, cz, bx, by, bz);
    const int b0[3] = {bx * f, by * f, bz * f};
    const int fshift = brick_shift(f);
    const uint32_t words = (uint32_t)(f * f * f) >> 5, vecs = words >> 2, nbits = words << 5;
    const uint32_t slot = meta[cell].x;
    for (uint32_t v = threadIdx.x; v < vecs; v += blockDim.x)
        old_vecs[v] = slot == kEmptySlot ? make_uint4(0u, 0u, 0u, 0u) : pool[(size_t)slot * vecs + v];
    if (threadIdx.x < 3)
        red[threadIdx.x] = 0x7FFFFFFF;
    else if (threadIdx.x < 6)
        red[threadIdx.x] = -1;
    else if (threadIdx.x < 8)
        red[threadIdx.x] = 0;
    if (threadIdx.x == 0)
        first = 0;
    __syncthreads();

    // the ops whose box meets the brick, and the last one that covers all of it
    for (uint32_t k = threadIdx.x; k < nops; k += blockDim.x) {
        const bool m = edit_meets_brick(ops[k], b0, f);
        meets[k] = m ? 1 : 0;
        if (m && edit_covers_brick(ops[k], b0, f))
            atomicMax(&first, (int)k);
    }
    __syncthreads();
    if (threadIdx.x < 64) {  // wave 0 compacts them in order: ballot + prefix count per 64 ops
        const uint32_t lane = threadIdx.x;
        uint32_t cnt = 0;
        for (uint32_t base = (uint32_t)first; base < nops; base += 64u) {
            const uint32_t k = base + lane;
            const bool m = k < nops && meets[k];
            const unsigned long long mask = __ballot(m);
            if (m)
                list[cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)k;
            cnt += (uint32_t)__popcll(mask);
        }
        if (lane == 0)
            count = (int)cnt;
    }
    __syncthreads();

    // one voxel per lane, as k_fill_bricks: a wave's 64 consecutive bits are 64 / f whole x-rows of the brick (HBM order:
    // x, then z, then y) and the ballot mask IS that uint64 of the image
    const uint32_t* old_words = reinterpret_cast<const uint32_t*>(old_vecs);
    const unsigned long long* old64 = reinterpret_cast<const unsigned long long*>(old_vecs);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(scratch + (size_t)i * vecs);
    const int nf = count;
    const uint32_t lane = threadIdx.x & 63u;
    int mn[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, mx[3] = {-1, -1, -1};
    bool diff = false;
    for (uint32_t o = threadIdx.x; o < nbits; o += blockDim.x) {  // nbits is a multiple of 512: whole waves iterate
        const int lx = (int)(o & (uint32_t)(f - 1)), lz = (int)((o >> fshift) & (uint32_t)(f - 1)), ly = (int)(o >> (2 * fshift));
        bool solid = ((old_words[o >> 5] >> (o & 31u)) & 1u) != 0u;
        for (int k = 0; k < nf; ++k) {
            const EditOpDev& op = ops[list[k]];
            if (edit_covers(op, b0[0] + lx, b0[1] + ly, b0[2] + lz))
                solid = op.value != 0;
        }
        const unsigned long long mask = __ballot(solid);
        if (lane == 0) {
            dst[o >> 6] = mask;
            diff |= mask != old64[o >> 6];
        }
        if (solid) {
            mn[0] = min(mn[0], lx); mn[1] = min(mn[1], ly); mn[2] = min(mn[2], lz);
            mx[0] = max(mx[0], lx); mx[1] = max(mx[1], ly); mx[2] = max(mx[2], lz);
        }
    }
    if (mx[0] >= 0) {
        atomicMin(&red[0], mn[0]); atomicMin(&red[1], mn[1]); atomicMin(&red[2], mn[2]);
        atomicMax(&red[3], mx[0]); atomicMax(&red[4], mx[1]); atomicMax(&red[5], mx[2]);
        red[6] = 1;
    }
    if (diff)
        red[7] = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int rmn[3] = {red[0], red[1], red[2]}, rmx[3] = {red[3], red[4], red[5]};
        ext[i] = red[6] ? edit_pack_extents(rmn, rmx) : 0u;
        info[i] = make_uint2(slot, (uint32_t)red[6] | ((uint32_t)red[7] << 1));
    }
}

// blocks [0, n): the touched cells (plan kEditKeep = unchanged: nothing to do); blocks [n, n + nzero): freed slots to zero
__global__ __launch_bounds__(256) void k_edit_commit(const uint32_t* __restrict__ cells, const uint32_t* __restrict__ new_slot,
                                                     uint32_t n, const uint32_t* __restrict__ zero, uint32_t nzero,
                                                     const uint4* __restrict__ scratch, const uint32_t* __restrict__ ext,
                                                     uint4* __restrict__ pool, uint2* __restrict__ meta,
                                                     uint32_t* __restrict__ coarse, uint32_t vecs)
{
    const uint32_t b = blockIdx.x + blockIdx.y * gridDim.x;
    if (b >= n) {
        if (b >= n + nzero)
            return;
        uint4* dst = pool + (size_t)zero[b - n] * vecs;
        for (uint32_t v = threadIdx.x; v < vecs; v += blockDim.x)
            dst[v] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint32_t s = new_slot[b];
    if (s == kEditKeep)
        return;
    const uint32_t cell = cells[b];
    if (threadIdx.x == 0) {
        meta[cell] = make_uint2(s, s == kEmptySlot ? 0u : ext[b]);
        if (s == kEmptySlot)
            atomicAnd(&coarse[cell >> 5], ~(1u << (cell & 31u)));
        else
            atomicOr(&coarse[cell >> 5], 1u << (cell & 31u));
    }
    if (s == kEmptySlot)
        return;
    const uint4* src = scratch + (size_t)b * vecs;
    uint4* dst = pool + (size_t)s * vecs;
    for (uint32_t v = threadIdx.x; v < vecs; v += blockDim.x)
        dst[v] = src[v];
}

// compacting save: brick idx[b] of the pool to dst[b]
__global__ __launch_bounds__(256) void k_gather_bricks(const uint4* __restrict__ pool, const uint32_t* __restrict__ idx,
                                                       uint4* __restrict__ dst, uint32_t vecs)
{
    const uint4* src = pool + (size_t)idx[blockIdx.x] * vecs;
    uint4* out = dst + (size_t)blockIdx.x * vecs;
    for (uint32_t v = threadIdx.x; v < vecs; v += blockDim.x)
        out[v] = src[v];
}

// host entry points (vxrt_api.hip)
hipError_t edit_bricks(const uint32_t* cells, uint32_t n, const EditOpDev* ops, uint32_t nops, const uint2* meta,
                       const uint32_t* pool, uint32_t* scratch, uint32_t* ext, uint2* info, int f, int cx, int cz)
{
    hipLaunchKernelGGL(k_edit_bricks, grid_2d(n), dim3(256), 0, 0, cells, n, ops, nops, meta, (const uint4*)pool,
                       (uint4*)scratch, ext, info, f, cx, cz);
    return hipGetLastError();
}
hipError_t edit_commit(const uint32_t* cells, const uint32_t* new_slot, uint32_t n, const uint32_t* zero, uint32_t nzero,
                       const uint32_t* scratch, const uint32_t* ext, uint32_t* pool, uint2* meta, uint32_t* coarse, int f)
{
    hipLaunchKernelGGL(k_edit_commit, grid_2d((uint64_t)n + nzero), dim3(256), 0, 0, cells, new_slot, n, zero, nzero,
                       (const uint4*)scratch, ext, (uint4*)pool, meta, coarse, (uint32_t)(f * f * f / 128));
    return hipGetLastError();
}
hipError_t gather_bricks(const uint32_t* pool, const uint32_t* idx, uint32_t n, uint32_t* dst, int f)
{
    if (n)
        hipLaunchKernelGGL(k_gather_bricks, dim3(n), dim3(256), 0, 0, (const uint4*)pool, idx, (uint4*)dst,
                           (uint32_t)(f * f * f / 128));
    return hipGetLastError();
}

}  // namespace vxrt
