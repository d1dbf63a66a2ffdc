// vxrt_region.hip -- region readback and voxel stamps of the resident brickmap (include/vxrt.h, vxrt_read_region /
// vxrt_edit_stamps; host side in vxrt_api.hip, shared row logic in vxrt_region.hpp).
//
//   k_read_region   one lane per output word: its 32 x-consecutive voxels gathered from the bricks they cross (up to
//                   32 / f + 1), one cell record and one brick row per brick, funnel-shifted into place.  A wave is 64
//                   consecutive words of a row, or 64 / L rows of L <= 64 lanes each when a row is shorter (L = the row's
//                   words rounded up to a power of two); a workgroup's four waves then step through up to 32 consecutive z,
//                   so that the 32 z-rows one pool line holds (f = 32) are read by one CU within a few microseconds.
//                   Clipped to the world before any load: never reads outside a table.
//   k_stamp_bricks  one 256-thread workgroup per touched brick cell, in the structure of k_edit_bricks: the old image into
//                   LDS, the stamps that meet the brick filtered into LDS in order (from the last replace stamp that
//                   covers the whole brick), then one brick word per lane -- one row at f = 32, two at 16, four at 8 --
//                   evaluated row by row against that list, extents from the OR of the rows (x) and from which rows are
//                   non-zero (y, z).  Writes exactly k_edit_bricks' outputs; the commit is vxrt_edit.hip's.
#include "../../include/vxrt.h"
#include "vxrt_edit.hpp"
#include "vxrt_kernels.hpp"
#include "vxrt_region.hpp"

namespace vxrt {

static_assert(sizeof(StampDev) == 72, "stamp layout (the host copies it as bytes)");

struct ReadArgs {
    const uint2* meta;
    const uint32_t* pool;
    uint32_t* out;
    int f, lgf, cx, cz;
    int X, Y, Z;
    int o[3], d[3];
    uint32_t wpr;       // words per region row (< 2^27)
    uint32_t pad_mask;  // valid bits of a row's last word
    int lgL;            // log2 of the lanes per row (L <= 64)
    uint32_t nxc, nyg;  // 64-word chunks of a row (1 when L < 64); groups of 64 / L rows along y
    int zsteps;         // z iterations per wave: a workgroup covers 4 * zsteps consecutive z
};

__global__ __launch_bounds__(256) void k_read_region(const ReadArgs A)
{
    // block -> (x chunk, y group, z group); block-uniform divisions (scalar)
    const uint32_t b = blockIdx.x + blockIdx.y * gridDim.x;
    const uint32_t xc = b % A.nxc, t = b / A.nxc, yg = t % A.nyg, zg = t / A.nyg;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t L = 1u << A.lgL;
    const uint32_t xw = xc * 64u + (lane & (L - 1u));
    const uint32_t yl = yg * (64u >> A.lgL) + (lane >> A.lgL);
    if (xw >= A.wpr || (int)yl >= A.d[1])
        return;
    const int64_t x0 = (int64_t)A.o[0] + 32 * (int64_t)xw;
    const int64_t wy = (int64_t)A.o[1] + yl;
    const bool y_in = wy >= 0 && wy < A.Y;
    const uint32_t mask = xw == A.wpr - 1u ? A.pad_mask : 0xFFFFFFFFu;
    // x clipped once: a word whose 32 voxels miss the world is 0 (no load)
    const bool x_in = x0 + 31 >= 0 && x0 < A.X;
    uint32_t zl = zg * (4u * (uint32_t)A.zsteps) + wave;
    uint64_t idx = ((uint64_t)yl + (uint64_t)A.d[1] * zl) * A.wpr + xw;
    const uint64_t step = (uint64_t)A.d[1] * 4u * A.wpr;
    for (int i = 0; i < A.zsteps && (int)zl < A.d[2]; ++i, zl += 4u, idx += step) {
        const int64_t wz = (int64_t)A.o[2] + zl;
        uint32_t w = 0u;
        if (y_in && x_in && wz >= 0 && wz < A.Z)
            w = region_row_word(A.meta, A.pool, A.f, A.lgf, A.cx, A.cz, x0, (int)wy, (int)wz);
        A.out[idx] = w & mask;
    }
}

__global__ __launch_bounds__(256) void k_stamp_bricks(const uint32_t* __restrict__ cells, uint32_t n,
                                                      const StampDev* __restrict__ stamps, uint32_t nst,
                                                      const uint2* __restrict__ meta, const uint4* __restrict__ pool,
                                                      uint32_t* __restrict__ scratch, uint32_t* __restrict__ ext,
                                                      uint2* __restrict__ info, int f, int cx, int cz)
{
    __shared__ uint4 old_vecs[256];  // the old image, f <= 32: 4 KiB
    __shared__ uint16_t list[kEditMaxOps];
    __shared__ uint8_t meets[kEditMaxOps];
    __shared__ int red[8];  // min y, min z, max y, max z, x bits (OR of the rows), changed
    __shared__ int first, count;
    const uint32_t i = blockIdx.x + blockIdx.y * gridDim.x;  // 2-D grid: more cells than one grid axis holds
    if (i >= n)
        return;
    const uint32_t cell = cells[i];
    int bx, by, bz;
    hbm_cell(cell, cx, cz, bx, by, bz);
    const int b0[3] = {bx * f, by * f, bz * f};
    const int lgf = brick_shift(f);
    const uint32_t words = (uint32_t)(f * f * f) >> 5, vecs = words >> 2;
    const uint32_t slot = meta[cell].x;
    for (uint32_t v = threadIdx.x; v < vecs; v += blockDim.x)
        old_vecs[v] = slot == kEmptySlot ? make_uint4(0u, 0u, 0u, 0u) : pool[(size_t)slot * vecs + v];
    if (threadIdx.x < 2)
        red[threadIdx.x] = 0x7FFFFFFF;
    else if (threadIdx.x < 4)
        red[threadIdx.x] = -1;
    else if (threadIdx.x < 8)
        red[threadIdx.x] = 0;
    if (threadIdx.x == 0)
        first = 0;
    __syncthreads();

    // the stamps whose box meets the brick, and the last replace stamp that covers all of it
    for (uint32_t k = threadIdx.x; k < nst; k += blockDim.x) {
        const bool m = stamp_meets_brick(stamps[k], b0, f);
        meets[k] = m ? 1 : 0;
        if (m && stamp_covers_brick(stamps[k], b0, f))
            atomicMax(&first, (int)k);
    }
    __syncthreads();
    if (threadIdx.x < 64) {  // wave 0 compacts them in order: ballot + prefix count per 64 stamps
        const uint32_t lane = threadIdx.x;
        uint32_t cnt = 0;
        for (uint32_t base = (uint32_t)first; base < nst; base += 64u) {
            const uint32_t k = base + lane;
            const bool m = k < nst && meets[k];
            const unsigned long long mask = __ballot(m);
            if (m)
                list[cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)k;
            cnt += (uint32_t)__popcll(mask);
        }
        if (lane == 0)
            count = (int)cnt;
    }
    __syncthreads();

    // one brick word per lane: 32 / f rows (row q = lz + f * ly, HBM order), each stepped through the stamp list
    const uint32_t* old_words = reinterpret_cast<const uint32_t*>(old_vecs);
    uint32_t* dst = scratch + (size_t)i * words;
    const int nf = count, rpw = 32 >> lgf;
    const uint32_t fmask = f == 32 ? 0xFFFFFFFFu : (1u << f) - 1u;
    int mn[2] = {0x7FFFFFFF, 0x7FFFFFFF}, mx[2] = {-1, -1};
    uint32_t xbits = 0u;
    bool diff = false;
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
        const uint32_t old = old_words[w];
        uint32_t img = 0u;
        for (int s = 0; s < rpw; ++s) {
            const uint32_t q = w * (uint32_t)rpw + (uint32_t)s;
            const int lz = (int)(q & (uint32_t)(f - 1)), ly = (int)(q >> lgf);
            uint32_t row = (old >> (s * f)) & fmask;
            for (int k = 0; k < nf; ++k)
                row = stamp_row(stamps[list[k]], b0, f, ly, lz, row);
            img |= row << (s * f);
            if (row) {
                xbits |= row;
                mn[0] = min(mn[0], ly); mn[1] = min(mn[1], lz);
                mx[0] = max(mx[0], ly); mx[1] = max(mx[1], lz);
            }
        }
        dst[w] = img;
        diff |= img != old;
    }
    if (xbits) {
        atomicMin(&red[0], mn[0]); atomicMin(&red[1], mn[1]);
        atomicMax(&red[2], mx[0]); atomicMax(&red[3], mx[1]);
        atomicOr(&red[4], (int)xbits);
    }
    if (diff)
        red[5] = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t xb = (uint32_t)red[4];
        const bool any = xb != 0u;
        if (any) {
            const int emn[3] = {__builtin_ctz(xb), red[0], red[1]}, emx[3] = {31 - __builtin_clz(xb), red[2], red[3]};
            ext[i] = edit_pack_extents(emn, emx);
        } else {
            ext[i] = 0u;
        }
        info[i] = make_uint2(slot, (uint32_t)any | ((uint32_t)red[5] << 1));
    }
}

// host entry points (vxrt_api.hip)
hipError_t read_region(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t* out, hipStream_t stream)
{
    ReadArgs A{};
    A.meta = W.meta;
    A.pool = W.pool;
    A.out = out;
    A.f = W.f;
    A.lgf = W.lgf;
    A.cx = W.cx;
    A.cz = W.cz;
    A.X = W.dim[0];
    A.Y = W.dim[1];
    A.Z = W.dim[2];
    for (int k = 0; k < 3; ++k) {
        A.o[k] = o[k];
        A.d[k] = d[k];
    }
    A.wpr = (uint32_t)region_words_per_row(d[0]);
    A.pad_mask = row_last_mask(d[0]);
    A.lgL = 0;
    while ((1u << A.lgL) < A.wpr && A.lgL < 6)
        ++A.lgL;
    A.nxc = (A.wpr + 63u) / 64u;
    const uint32_t rows_per_wave = 64u >> A.lgL;
    A.nyg = (uint32_t)(((uint64_t)d[1] + rows_per_wave - 1) / rows_per_wave);
    // z per workgroup: up to 32 (8 steps of 4 waves), fewer while that leaves under 2048 workgroups (8 per CU)
    const uint64_t xy = (uint64_t)A.nxc * A.nyg;
    A.zsteps = 8;
    while (A.zsteps > 1 && xy * (((uint64_t)d[2] + 4u * A.zsteps - 1) / (4u * A.zsteps)) < 2048u)
        A.zsteps >>= 1;
    const uint64_t blocks = xy * (((uint64_t)d[2] + 4u * A.zsteps - 1) / (4u * A.zsteps));
    if (blocks >= (1ull << 32))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_read_region, grid_2d(blocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t stamp_bricks(const uint32_t* cells, uint32_t n, const StampDev* stamps, uint32_t nst, const uint2* meta,
                        const uint32_t* pool, uint32_t* scratch, uint32_t* ext, uint2* info, int f, int cx, int cz)
{
    hipLaunchKernelGGL(k_stamp_bricks, grid_2d(n), dim3(256), 0, 0, cells, n, stamps, nst, meta, (const uint4*)pool, scratch,
                       ext, info, f, cx, cz);
    return hipGetLastError();
}

}  // namespace vxrt
