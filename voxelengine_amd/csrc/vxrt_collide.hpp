// vxrt_collide.hpp -- batched box collision queries (include/vxrt.h, vxrt_move_boxes / vxrt_overlap_boxes): the pieces
// shared by the kernels of vxrt_collide.hip and the host harness of the tests (tests/tools/collide_check.cpp, through
// tests/tools/hoststub): body validation, the voxel ranges a box overlaps, the slab search of one axis, the snap arithmetic
// and the overlap count.  Every voxel row is gathered with region_row_word (vxrt_region.hpp), whose cell-record test skips
// empty bricks before any pool load.
//
// Float arithmetic: the only float operations are the additions and subtractions of the contract (no product, so nothing
// a compiler could contract into an FMA; the library and the harness build with -ffp-contract=off all the same), floorf /
// ceilf and int -> float conversions, all exact or correctly rounded binary32 on host and device alike.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vxrt_device.hpp"
#include "vxrt_region.hpp"

// The harness defines this to check, before every row gather, that the row lies inside the world and that the cell records
// the gather reads lie inside the cell table.  The kernels leave it empty: the ranges are clipped to the world first.
#ifndef VXRT_COLLIDE_CHECK_ROW
#define VXRT_COLLIDE_CHECK_ROW(W, x0, y, z)
#endif

namespace vxrt {

constexpr int kBodyMaxExtent = 64;      // VXRT_BODY_MAX_EXTENT
constexpr int kBodyMaxDelta = 64;       // VXRT_BODY_MAX_DELTA
constexpr float kBodyMaxCoord = 16777216.0f;  // 2^24: |lo|, |hi| stay below it
constexpr uint32_t kBodyInvalid = 8u;   // VXRT_BODY_INVALID

// the body rule of include/vxrt.h: finite, lo < hi, hi - lo <= 64, |delta| <= 64, |lo|, |hi| < 2^24 on every axis
__host__ __device__ inline bool body_valid(const float b[9])
{
    for (int k = 0; k < 3; ++k) {
        const float lo = b[k], hi = b[3 + k], d = b[6 + k];
        // every comparison with a NaN is false, an infinity fails the magnitude bounds
        if (!(lo > -kBodyMaxCoord && lo < kBodyMaxCoord && hi > -kBodyMaxCoord && hi < kBodyMaxCoord))
            return false;
        if (!(lo < hi) || !(hi - lo <= (float)kBodyMaxExtent))
            return false;
        if (!(d >= -(float)kBodyMaxDelta && d <= (float)kBodyMaxDelta))
            return false;
    }
    return true;
}

// the voxels [floor(lo), ceil(hi) - 1] a box overlaps on one axis, clipped to [0, n - 1] (empty: r0 > r1)
__host__ __device__ inline void cover_range(float lo, float hi, int n, int& r0, int& r1)
{
    const int a = (int)floorf(lo), b = (int)ceilf(hi) - 1;
    r0 = a < 0 ? 0 : a;
    r1 = b > n - 1 ? n - 1 : b;
}

__host__ __device__ inline uint32_t collide_row(const CollideWorld& W, int64_t x0, int y, int z)
{
    VXRT_COLLIDE_CHECK_ROW(W, x0, y, z);
    return region_row_word(W.meta, W.pool, W.f, W.lgf, W.cx, W.cz, x0, y, z);
}

// whether row (y, z) holds a solid voxel in x in [x0, x1] (0 <= x0 <= x1 < dim[0])
__host__ __device__ inline bool row_any(const CollideWorld& W, int x0, int x1, int y, int z)
{
    for (int xs = x0; xs <= x1; xs += 32) {
        const int top = x1 - xs > 31 ? 31 : x1 - xs;
        if (collide_row(W, xs, y, z) & bit_range(0, top))
            return true;
    }
    return false;
}

// the least (dir > 0) or greatest (dir < 0) x in [s0, s1] at which a row (y, z) of the cross-section [y0, y1] x [z0, z1]
// holds a solid voxel, or `none`.  One row word answers 32 slabs: masked to the slabs still open, then its first or last
// set bit; the open range shrinks to the best found so far.
__host__ __device__ inline int search_x(const CollideWorld& W, int s0, int s1, int y0, int y1, int z0, int z1, int dir, int none)
{
    int best = none;
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            if (s0 > s1)
                return best;
            if (dir > 0) {
                for (int xs = s0; xs <= s1; xs += 32) {
                    const int top = s1 - xs > 31 ? 31 : s1 - xs;
                    const uint32_t w = collide_row(W, xs, y, z) & bit_range(0, top);
                    if (w) {
                        best = xs + __builtin_ctz(w);
                        s1 = best - 1;
                        break;
                    }
                }
            } else {
                for (int xe = s1; xe >= s0; xe -= 32) {  // word of the voxels xe - 31 .. xe
                    const int bot = s0 - (xe - 31) > 0 ? s0 - (xe - 31) : 0;
                    const uint32_t w = collide_row(W, (int64_t)xe - 31, y, z) & bit_range(bot, 31);
                    if (w) {
                        best = xe - 31 + (31 - __builtin_clz(w));
                        s0 = best + 1;
                        break;
                    }
                }
            }
        }
    return best;
}

// the nearest slab v of [s0, s1] along axis a (1 = y, 2 = z) in direction dir that holds a solid voxel within the cross-
// section r0 / r1 of the other two axes (x in words of 32), or `none`; slabs are tested nearest first and the search stops
// at the first solid one
__host__ __device__ inline int search_yz(const CollideWorld& W, int a, int s0, int s1, const int r0[3], const int r1[3], int dir,
                                         int none)
{
    const int b = a == 1 ? 2 : 1;  // the other row axis
    const int n = s1 - s0 + 1;
    for (int i = 0; i < n; ++i) {
        const int v = dir > 0 ? s0 + i : s1 - i;
        for (int u = r0[b]; u <= r1[b]; ++u) {
            const int y = a == 1 ? v : u, z = a == 1 ? u : v;
            if (row_any(W, r0[0], r1[0], y, z))
                return v;
        }
    }
    return none;
}

// the nearest solid slab of [s0, s1] on axis a in direction dir (s0 / s1 already clipped to the world), or `none`
__host__ __device__ inline int nearest_solid(const CollideWorld& W, int a, int s0, int s1, const int r0[3], const int r1[3],
                                             int dir, int none)
{
    for (int k = 0; k < 3; ++k)  // an empty cross-section (the ranges of axis a itself are not used)
        if (k != a && r0[k] > r1[k])
            return none;
    if (s0 > s1)
        return none;
    if (a == 0)
        return search_x(W, s0, s1, r0[1], r1[1], r0[2], r1[2], dir, none);
    return search_yz(W, a, s0, s1, r0, r1, dir, none);
}

// One body moved axis by axis in `order` (include/vxrt.h, vxrt_move_boxes): lo / hi updated in place, the blocked bits
// returned.  The body must be valid (body_valid).
__host__ __device__ inline uint32_t move_body(const CollideWorld& W, float lo[3], float hi[3], const float delta[3],
                                              const int order[3])
{
    uint32_t flags = 0u;
    for (int i = 0; i < 3; ++i) {
        const int a = order[i];
        const float d = delta[a];
        if (d == 0.0f)  // -0 included
            continue;
        int r0[3], r1[3];
        for (int k = 0; k < 3; ++k)
            cover_range(lo[k], hi[k], W.dim[k], r0[k], r1[k]);
        const int n = W.dim[a];
        if (d > 0.0f) {
            const float e = hi[a] + d;
            int s0 = (int)ceilf(hi[a]), s1 = (int)ceilf(e) - 1;
            s0 = s0 < 0 ? 0 : s0;
            s1 = s1 > n - 1 ? n - 1 : s1;
            const int F = nearest_solid(W, a, s0, s1, r0, r1, +1, INT32_MIN);
            if (F != INT32_MIN) {
                const float ff = (float)F;
                lo[a] = lo[a] + (ff - hi[a]);
                hi[a] = ff;
                flags |= 1u << a;
            } else {
                lo[a] = lo[a] + d;
                hi[a] = e;
            }
        } else {
            const float e = lo[a] + d;
            int s0 = (int)floorf(e), s1 = (int)floorf(lo[a]) - 1;
            s0 = s0 < 0 ? 0 : s0;
            s1 = s1 > n - 1 ? n - 1 : s1;
            const int G = nearest_solid(W, a, s0, s1, r0, r1, -1, INT32_MIN);
            if (G != INT32_MIN) {
                const float g1 = (float)(G + 1);
                hi[a] = hi[a] + (g1 - lo[a]);
                lo[a] = g1;
                flags |= 1u << a;
            } else {
                lo[a] = e;
                hi[a] = hi[a] + d;
            }
        }
    }
    return flags;
}

// the solid voxels of [floor(lo), ceil(hi) - 1] on all three axes (include/vxrt.h, vxrt_overlap_boxes)
__host__ __device__ inline uint32_t overlap_count(const CollideWorld& W, const float lo[3], const float hi[3])
{
    int r0[3], r1[3];
    for (int k = 0; k < 3; ++k)
        cover_range(lo[k], hi[k], W.dim[k], r0[k], r1[k]);
    uint32_t count = 0u;
    if (r0[0] > r1[0] || r0[1] > r1[1] || r0[2] > r1[2])
        return 0u;
    for (int z = r0[2]; z <= r1[2]; ++z)
        for (int y = r0[1]; y <= r1[1]; ++y)
            for (int xs = r0[0]; xs <= r1[0]; xs += 32) {
                const int top = r1[0] - xs > 31 ? 31 : r1[0] - xs;
                count += (uint32_t)__builtin_popcount(collide_row(W, xs, y, z) & bit_range(0, top));
            }
    return count;
}

// the whole per-body step of the two kernels: validation, then the move (lohi_out: lo[3], hi[3]) or the count
__host__ __device__ inline uint32_t collide_move_one(const CollideWorld& W, const float b[9], const int order[3], float out[6])
{
    for (int k = 0; k < 6; ++k)
        out[k] = b[k];
    if (!body_valid(b))
        return kBodyInvalid;
    return move_body(W, out, out + 3, b + 6, order);
}

__host__ __device__ inline uint32_t collide_overlap_one(const CollideWorld& W, const float b[9], uint32_t& flags)
{
    if (!body_valid(b)) {
        flags = kBodyInvalid;
        return 0u;
    }
    flags = 0u;
    return overlap_count(W, b, b + 3);
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_collide.hip on n bodies
hipError_t move_boxes(const CollideWorld& W, const float* bodies, uint64_t n, const int order[3], float* lohi, uint32_t* flags,
                      hipStream_t stream);
hipError_t overlap_boxes(const CollideWorld& W, const float* bodies, uint64_t n, uint32_t* counts, uint32_t* flags,
                         hipStream_t stream);
#endif

}  // namespace vxrt
