// vxrt_region.hpp -- region readback and voxel stamps (include/vxrt.h, vxrt_read_region / vxrt_edit_stamps): the pieces
// shared by the kernels of vxrt_region.hip, the host side in vxrt_api_query.hip and the host harnesses of the tests
// (tests/tools/*_check.cpp, through tests/tools/hoststub): the brick row, the 32-voxel row gather of a read, the
// funnel-shifted gather of a stamp's bits, the per-row stamp step, the per-brick stamp filter and stamp validation.
// Every world query (edits, reads, collision, islands, navigation, distance, surface, LOD, light, rules) reads the world
// through this layer, so it also holds what they share:
//   host (also under VXRT_HOST_CHECK)  the world as a query reads it; workspace sections and their cursor (Sections); the box
//                                      contract of a query (box_voxels) and of its halo (halo_box, HaloBox, BoxFault); the
//                                      mask of a bit row's last word (row_last_mask)
//   device                             the 2-D launch grid with its flat ids (grid_2d, flat_block, flat_thread), the wave
//                                      sum, min and max, and the atomics
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_device.hpp"
#include "../../include/vxrt.h"  // the table and summary types in the signatures of the query families' launchers

namespace vxrt {

constexpr uint64_t kRegionMaxVoxels = 1ull << 36;

// the resident world as a query reads it (HBM order, vxrt_device.hpp).  Named after its first user, the collision
// queries: the name is part of the collision kernels' symbols and of what the collision harness declares.
struct CollideWorld {
    const uint2* meta;
    const uint32_t* pool;
    int f, lgf, cx, cz;
    int dim[3];  // voxels per axis
};

// the world of f-voxel bricks, cd cells per axis
inline CollideWorld query_world(const uint2* meta, const uint32_t* pool, int f, const int cd[3])
{
    CollideWorld W{};
    W.meta = meta;
    W.pool = pool;
    W.f = f;
    W.lgf = brick_shift(f);
    W.cx = cd[0];
    W.cz = cd[2];
    for (int k = 0; k < 3; ++k)
        W.dim[k] = cd[k] * f;
    return W;
}

// n rounded up to a multiple of 256 bytes, n counted in units of `unit` bytes: workspace and scratch sections start on
// 256-byte boundaries
inline uint64_t section_up(uint64_t n, uint64_t unit = 1)
{
    const uint64_t a = 256u / unit;
    return (n + a - 1u) / a * a;
}

// the sections of a workspace in turn: take() returns the offset of the next one and moves past it.  Offsets count units of
// `unit` bytes (one layout, one unit)
struct Sections {
    uint64_t at = 0;
    uint64_t take(uint64_t n, uint64_t unit = 1)
    {
        const uint64_t o = at;
        at += section_up(n, unit);
        return o;
    }
};

#ifndef VXRT_HOST_CHECK
// more workgroups than one grid axis holds: x up to 2^20, the rest in y (the kernels flatten it again: flat_block)
inline dim3 grid_2d(uint64_t blocks)
{
    const unsigned gx = blocks > (1u << 20) ? (1u << 20) : (unsigned)(blocks ? blocks : 1);
    return dim3(gx, (unsigned)((blocks + gx - 1) / gx));
}
// the workgroup's number in a grid_2d launch, and the lane's with 256-lane workgroups
__device__ inline uint64_t flat_block() { return (uint64_t)blockIdx.x + (uint64_t)blockIdx.y * gridDim.x; }
__device__ inline uint64_t flat_thread() { return flat_block() * 256u + threadIdx.x; }

// k_read_region of the box o, d into `out` (region layout); vxrt_region.hip
hipError_t read_region(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t* out, hipStream_t stream);
// k_stamp_bricks: the stamps (StampDev, below) applied to the touched cells, in k_edit_bricks' output format (vxrt_edit.hpp)
hipError_t stamp_bricks(const uint32_t* cells, uint32_t n, const struct StampDev* stamps, uint32_t nst, const uint2* meta,
                        const uint32_t* pool, uint32_t* scratch, uint32_t* ext, uint2* info, int f, int cx, int cz);

__device__ inline uint32_t wave_sum(uint32_t v)
{
    for (int m = 32; m; m >>= 1)
        v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ inline uint32_t wave_max(uint32_t v)
{
    for (int m = 32; m; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline int32_t wave_min(int32_t v)
{
    for (int m = 32; m; m >>= 1) {
        const int32_t o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline int32_t wave_max(int32_t v)
{
    for (int m = 32; m; m >>= 1) {
        const int32_t o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}
#endif

// Atomics of the query kernels, each returning the old value.  On the host every "atomic" is a plain read-modify-write: the
// harnesses run one lane at a time.
#if defined(__HIP_DEVICE_COMPILE__)
// agent-scope loads: another CU's atomic is seen, not a stale line of this CU's L1
__device__ inline uint32_t atom_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T>
__device__ inline T atom_min(T* p, T v) { return atomicMin(p, v); }
template <class T>
__device__ inline T atom_max(T* p, T v) { return atomicMax(p, v); }
__device__ inline uint32_t atom_or(uint32_t* p, uint32_t v) { return atomicOr(p, v); }
__device__ inline uint32_t atom_add(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
__device__ inline uint64_t atom_add64(uint64_t* p, uint64_t v) { return atomicAdd((unsigned long long*)p, (unsigned long long)v); }
#else
inline uint32_t atom_load(const uint32_t* p) { return *p; }
template <class T>
inline T atom_min(T* p, T v)
{
    const T o = *p;
    if (v < o)
        *p = v;
    return o;
}
template <class T>
inline T atom_max(T* p, T v)
{
    const T o = *p;
    if (v > o)
        *p = v;
    return o;
}
inline uint32_t atom_or(uint32_t* p, uint32_t v)
{
    const uint32_t o = *p;
    *p = o | v;
    return o;
}
inline uint32_t atom_add(uint32_t* p, uint32_t v)
{
    const uint32_t o = *p;
    *p = o + v;
    return o;
}
inline uint64_t atom_add64(uint64_t* p, uint64_t v)
{
    const uint64_t o = *p;
    *p = o + v;
    return o;
}
#endif

// a stamp as the kernels read it: validated, its voxel box clipped to the world (lo > hi on some axis: a no-op)
struct StampDev {
    const uint32_t* bits;  // device, region layout (include/vxrt.h)
    uint64_t wpr;          // words per row: ceil(d[0] / 32)
    int32_t o[3], d[3];    // origin and dims, as given
    int32_t lo[3], hi[3];  // the stamp's box clipped to the world, inclusive
    int32_t mode, pad_;    // vxrt_stamp_mode
};

// the voxels of a box of dims d; 0 outside the contract: each dim at least 1, at most max_voxels (below 2^62) in all
inline uint64_t box_voxels(const int32_t d[3], uint64_t max_voxels)
{
    if (d[0] < 1 || d[1] < 1 || d[2] < 1)
        return 0;
    const uint64_t v01 = (uint64_t)d[0] * (uint64_t)d[1];  // < 2^62
    if (v01 > max_voxels || (uint64_t)d[2] > max_voxels / v01)
        return 0;
    return v01 * (uint64_t)d[2];
}

// words of a region row, and of a region; 0 for dims outside the contract
__host__ __device__ inline uint64_t region_words_per_row(int32_t d0) { return ((uint64_t)d0 + 31u) >> 5; }
inline uint64_t region_words(const int32_t d[3])
{
    return box_voxels(d, kRegionMaxVoxels) ? region_words_per_row(d[0]) * (uint64_t)d[1] * (uint64_t)d[2] : 0;
}
// the bits of the last word of a region row of d0 voxels that are voxels (the rest is padding, kept 0)
__host__ __device__ inline uint32_t row_last_mask(int32_t d0) { return (d0 & 31) ? (1u << (d0 & 31)) - 1u : 0xFFFFFFFFu; }

// ---- the halo box of a query ----------------------------------------------------------------------------------------------
// why a box is refused: its dims (or its family's own limits), or where its origin puts it
enum BoxFault { kBoxOk = 0, kBoxDims, kBoxOrigin };

// The box o, d grown by h voxels on every side, as a region read holds it: the base of a family's layout.
struct HaloBox {
    BoxFault fault;        // set by the family's layout: what it returned false for
    int32_t ho[3], hd[3];  // origin (only when an origin was given) and dims of the halo box
    uint64_t nhalo;        // its region words
    uint32_t wh, hy, hz;   // words per halo row, halo rows, halo slices
};

// Fills H (but for H.fault) for 0 <= h < 2^16.  kBoxDims: d outside box_voxels' contract or a halo box beyond what a region
// read holds; kBoxOrigin (only when `o` is given, and only for dims within the contract): o - h or o + d + h beyond int32.
inline BoxFault halo_box(const int32_t* o, const int32_t d[3], int32_t h, uint64_t max_voxels, HaloBox& H)
{
    if (box_voxels(d, max_voxels) == 0)
        return kBoxDims;
    for (int k = 0; k < 3; ++k) {
        if ((int64_t)d[k] + 2 * (int64_t)h > INT32_MAX)
            return kBoxDims;
        H.hd[k] = d[k] + 2 * h;
    }
    H.nhalo = region_words(H.hd);
    if (H.nhalo == 0)
        return kBoxDims;
    for (int k = 0; o && k < 3; ++k) {
        if ((int64_t)o[k] - h < INT32_MIN || (int64_t)o[k] + d[k] + h > INT32_MAX)
            return kBoxOrigin;
        H.ho[k] = o[k] - h;
    }
    H.wh = (uint32_t)region_words_per_row(H.hd[0]);
    H.hy = (uint32_t)H.hd[1];
    H.hz = (uint32_t)H.hd[2];
    return kBoxOk;
}

// bits [0, f) of row (ly, lz) of a brick image (HBM order inside a brick: bit x + f * (z + f * y), a row is f bits)
__host__ __device__ inline uint32_t brick_row(const uint32_t* brick, int f, int ly, int lz)
{
    const uint32_t rb = (uint32_t)f * ((uint32_t)lz + (uint32_t)f * (uint32_t)ly);
    const uint32_t w = brick[rb >> 5];
    return f == 32 ? w : (w >> (rb & 31u)) & ((1u << f) - 1u);
}

// `bits` placed so that its bit 0 lands on bit d of the result, -32 < d < 32 (a funnel shift: v_alignbit)
__host__ __device__ inline uint32_t place_bits(uint32_t bits, int d)
{
    return (uint32_t)(((uint64_t)bits << (32 + d)) >> 32);
}

// The word of a region read for world row (y, z), voxels x0 .. x0 + 31: bit j = voxel x0 + j, 0 outside the world.  The
// row (y, z) must lie inside the world (the caller clips y and z); x is clipped to the bricks [0, cx) before any load.  The
// 32 voxels cross up to 32 / f + 1 bricks; per brick one cell record and one brick row, funnel-shifted into place.
__host__ __device__ inline uint32_t region_row_word(const uint2* meta, const uint32_t* pool, int f, int lgf, int cx, int cz,
                                                    int64_t x0, int y, int z)
{
    const int64_t bl = x0 >> lgf, bh = (x0 + 31) >> lgf;  // arithmetic shifts: floor for negative x0
    const int b_lo = bl < 0 ? 0 : (int)bl, b_hi = bh > cx - 1 ? cx - 1 : (int)bh;
    const int by = y >> lgf, bz = z >> lgf, ly = y & (f - 1), lz = z & (f - 1);
    const uint64_t row_cells = hbm_index(0, by, bz, cx, cz);
    const uint32_t bw = (uint32_t)(f * f * f) >> 5;
    uint32_t out = 0u;
    for (int bx = b_lo; bx <= b_hi; ++bx) {
        const uint32_t slot = meta[row_cells + (uint64_t)bx].x;
        if (slot == kEmptySlot)
            continue;
        const uint32_t r = brick_row(pool + (size_t)slot * bw, f, ly, lz);
        out |= place_bits(r, (int)((int64_t)bx * f - x0));
    }
    return out;
}

// the mask of the bits [a, b] of a word, 0 <= a <= b <= 31
__host__ __device__ inline uint32_t bit_range(int a, int b) { return (0xFFFFFFFFu >> (31 - b)) & (0xFFFFFFFFu << a); }

// the 32 bits sx .. sx + 31 of one region row of `nw` words (bit x of the row = bit x & 31 of word x >> 5); words outside
// [0, nw) read as 0 and are not loaded
__host__ __device__ inline uint32_t row_gather32(const uint32_t* row, uint64_t nw, int64_t sx)
{
    const int64_t k = sx >> 5;
    const int s = (int)(sx & 31);
    const uint32_t lo = (k >= 0 && (uint64_t)k < nw) ? row[k] : 0u;
    const uint32_t hi = (k + 1 >= 0 && (uint64_t)(k + 1) < nw) ? row[k + 1] : 0u;
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> s);
}

// the stamp's box meets the brick's voxel box [b0, b0 + f - 1]^3
__host__ __device__ inline bool stamp_meets_brick(const StampDev& s, const int b0[3], int f)
{
    for (int a = 0; a < 3; ++a)
        if (s.hi[a] < b0[a] || s.lo[a] > b0[a] + f - 1)
            return false;
    return true;
}

// the stamp decides every voxel of the brick whatever it held: a replace stamp whose box contains the brick
__host__ __device__ inline bool stamp_covers_brick(const StampDev& s, const int b0[3], int f)
{
    if (s.mode != 0)
        return false;
    for (int a = 0; a < 3; ++a)
        if (s.lo[a] > b0[a] || s.hi[a] < b0[a] + f - 1)
            return false;
    return true;
}

// one stamp applied to row (ly, lz) of the brick at voxel b0 (f bits, bit lx = voxel b0[0] + lx): the stamp's bits for the
// row gathered funnel-shifted, ANDed with the row's coverage (the stamp's clipped x-range within the brick), then
// replace: row = (row & ~c) | (m & c); union: row |= m & c; subtract: row &= ~(m & c)
__host__ __device__ inline uint32_t stamp_row(const StampDev& s, const int b0[3], int f, int ly, int lz, uint32_t row)
{
    const int wy = b0[1] + ly, wz = b0[2] + lz;
    if (wy < s.lo[1] || wy > s.hi[1] || wz < s.lo[2] || wz > s.hi[2])
        return row;
    const int xa = s.lo[0] > b0[0] ? s.lo[0] : b0[0];
    const int xb = s.hi[0] < b0[0] + f - 1 ? s.hi[0] : b0[0] + f - 1;
    if (xa > xb)
        return row;
    const uint32_t c = bit_range(xa - b0[0], xb - b0[0]);
    const uint64_t r = (uint64_t)((int64_t)wy - s.o[1]) + (uint64_t)s.d[1] * (uint64_t)((int64_t)wz - s.o[2]);
    const uint32_t m = row_gather32(s.bits + r * s.wpr, s.wpr, (int64_t)b0[0] - s.o[0]) & c;
    if (s.mode == 0)
        return (row & ~c) | m;
    if (s.mode == 1)
        return row | m;
    return row & ~m;
}

// ---- host: stamp validation and clipping ---------------------------------------------------------------------------
// 0 = valid; X, Y, Z = world voxels per axis.  *noop = the stamp's box misses the world.
inline int stamp_prepare(const uint32_t* bits, const int32_t o[3], const int32_t d[3], int32_t mode, int32_t reserved, int X,
                         int Y, int Z, StampDev& out, bool& noop)
{
    if (!(mode == 0 || mode == 1 || mode == 2) || reserved != 0 || !bits || region_words(d) == 0)
        return -1;
    const int64_t dim[3] = {X, Y, Z};
    out = StampDev{};
    out.bits = bits;
    out.wpr = region_words_per_row(d[0]);
    out.mode = mode;
    noop = false;
    for (int k = 0; k < 3; ++k) {
        int64_t lo = o[k], hi = (int64_t)o[k] + d[k] - 1;
        lo = lo < 0 ? 0 : lo;
        hi = hi > dim[k] - 1 ? dim[k] - 1 : hi;
        if (lo > hi) {
            noop = true;
            lo = 1;
            hi = 0;
        }
        out.o[k] = o[k];
        out.d[k] = d[k];
        out.lo[k] = (int32_t)lo;
        out.hi[k] = (int32_t)hi;
    }
    return 0;
}

}  // namespace vxrt
