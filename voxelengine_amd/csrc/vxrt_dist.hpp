// vxrt_dist.hpp -- exact distance fields (include/vxrt.h, vxrt_distance_field): the pieces shared by the kernels of
// vxrt_dist.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/dist_check.cpp, through
// tests/tools/hoststub): the workspace layout, the x distance of one voxel from the halo's bits, the min-plus scan of one
// column of a slab, the loads and stores of the two sweeps, the occupancy cells and live tiles of the empty-space skip
// and the summary tally.
//
// Halo.  The targets within R of the voxels of B lie in the box [origin - R, origin + dims + R) of the world: halo voxel
// (hx, hy, hz) is world voxel origin - R + (hx, hy, hz), so voxel (x, y, z) of B is halo voxel (x + R, y + R, z + R).  Its
// bits come from k_read_region (outside the world: 0); VXRT_DIST_TO_EMPTY reads them inverted, a row's padding bits kept 0.
// Separable squared distance.  d2(v) = min over dz of (min over dy of (min over dx of dx^2) + dy^2) + dz^2, every offset
// within [-R, R]; a partial sum above R^2 is stored as FAR (it can only end above R^2).  Three dependent sweeps:
//   x   from the bits: the nearest set bit at or below and at or above the voxel, by count-leading / count-trailing zeros on
//       the voxel's word and at most ceil(R / 32) + 1 words each way.  Computed where the y sweep loads it, never stored.
//   y   g2(x, y, hz) for the rows y of B and every halo slice hz: one column slab of 64 x (64 + 2R) x-distances in LDS, the
//       scan of one output running outwards from k = 0 and stopping when k^2 >= the best so far.
//   z   the same scan over g2 along z: the output, cut at R^2, and the summary.
// Empty-space skip.  A tile is 64 x 64 x 64 voxels of B.  A tile whose halo neighbourhood (the tile grown by R on every
// axis) holds no target is not live: its voxels are FAR, the z sweep fills them, and the y sweep leaves out every slice
// that only tiles that are not live would read.  Occupancy is kept per cell of 32 x 8 x 8 halo voxels (one region word, 8
// rows, 8 slices).  It changes no value: a voxel of a tile that is not live has no target within R on every axis.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into an array of the workspace, the outputs or a slab
// against that array's size (array: one of the kDist* ids below).  The kernels leave it empty.
#ifndef VXRT_DIST_CHECK
#define VXRT_DIST_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint64_t kDistMaxVoxels = 1ull << 28;
constexpr uint32_t kDistMaxRadius = 255, kDistFar = 0xFFFFu;
constexpr uint32_t kDistTile = 64;  // a tile is 64 x 64 x 64 voxels; a slab column serves 64 outputs
constexpr uint32_t kDistCell = 8;   // an occupancy cell is one halo word x 8 rows x 8 slices
constexpr uint32_t kDistRows = 8;   // rows of B one z-sweep workgroup takes in turn (divides kDistTile)
enum { kDistHalo, kDistG2, kDistOcc, kDistLive, kDistOut, kDistSlab };
// summary words (vxrt_distance_summary); sum_d2 is the uint64 at words 4 and 5
enum { kDistSumZero, kDistSumNear, kDistSumFar, kDistSumMax, kDistSumSum };

// the workspace: sections of bytes, each on a 256-byte boundary (include/vxrt.h states the same formula)
struct DistLayout : HaloBox {      // the halo box (vxrt_region.hpp): B grown by the radius
    uint64_t halo, g2, occ, live;  // byte offsets
    uint64_t total_bytes;
    uint64_t ng2, nocc;         // g2 cells, occupancy cells
    uint32_t nvox;              // voxels of B
    uint32_t ncy, ncz;          // occupancy cells along y and z (wh along x)
    uint32_t ntx, nty, ntz, ntiles;
};

// false outside the contract (L.fault: why): radius, dims, the halo box within a region read and, when `o` is given, within
// int32
inline bool dist_layout(const int32_t* o, const int32_t d[3], uint32_t r, DistLayout& L)
{
    L.fault = r < 1 || r > kDistMaxRadius ? kBoxDims : halo_box(o, d, (int32_t)r, kDistMaxVoxels, L);
    if (L.fault != kBoxOk)
        return false;
    L.nvox = (uint32_t)box_voxels(d, kDistMaxVoxels);
    L.ng2 = (uint64_t)d[0] * (uint64_t)d[1] * L.hz;
    L.ncy = (L.hy + kDistCell - 1) / kDistCell;
    L.ncz = (L.hz + kDistCell - 1) / kDistCell;
    L.nocc = (uint64_t)L.wh * L.ncy * L.ncz;
    L.ntx = ((uint32_t)d[0] + kDistTile - 1) / kDistTile;
    L.nty = ((uint32_t)d[1] + kDistTile - 1) / kDistTile;
    L.ntz = ((uint32_t)d[2] + kDistTile - 1) / kDistTile;
    L.ntiles = L.ntx * L.nty * L.ntz;
    Sections S;
    L.halo = S.take(4u * L.nhalo);
    L.g2 = S.take(2u * L.ng2);
    L.occ = S.take(L.nocc);
    L.live = S.take(L.ntiles);
    L.total_bytes = S.at;
    return true;
}

// what the distance kernels read and write (device pointers; host pointers in the harness)
struct DistArgs {
    const uint32_t* halo;  // the halo's region words (k_read_region)
    uint16_t* g2;          // x + dims[0] * (y + dims[1] * hz): after the y sweep
    uint8_t* occ;          // xw + wh * (cy + ncy * cz): the cell holds a target
    uint8_t* live;         // tx + ntx * (ty + nty * tz): the tile's neighbourhood holds a target
    uint16_t* out;         // output: d_dist2
    uint32_t* summary;     // output: vxrt_distance_summary
    int32_t d[3];
    uint32_t r, r2, mode, skip;  // skip = 0: every tile is live (the harness's comparison run)
    uint32_t wh, hy, hz, ncy, ncz, ntx, nty, ntz;
};

inline void dist_args(DistArgs& A, const DistLayout& L, const int32_t d[3], uint32_t r, uint32_t mode, void* work, uint16_t* out,
                      uint32_t* summary)
{
    A.halo = (const uint32_t*)((char*)work + L.halo);
    A.g2 = (uint16_t*)((char*)work + L.g2);
    A.occ = (uint8_t*)work + L.occ;
    A.live = (uint8_t*)work + L.live;
    A.out = out;
    A.summary = summary;
    for (int k = 0; k < 3; ++k)
        A.d[k] = d[k];
    A.r = r;
    A.r2 = r * r;
    A.mode = mode;
    A.skip = 1u;
    A.wh = L.wh;
    A.hy = L.hy;
    A.hz = L.hz;
    A.ncy = L.ncy;
    A.ncz = L.ncz;
    A.ntx = L.ntx;
    A.nty = L.nty;
    A.ntz = L.ntz;
}

// ---- targets ----------------------------------------------------------------------------------------------------------

// word xw of halo row `row` (= hy + A.hy * hz) as target bits: the solid voxels, or the empty ones with the padding 0
__host__ __device__ inline uint32_t dist_targets(const DistArgs& A, uint64_t row, uint32_t xw)
{
    VXRT_DIST_CHECK(kDistHalo, row * A.wh + xw);
    const uint32_t w = A.halo[row * A.wh + xw];
    if (A.mode == 0u)
        return w;
    const uint32_t rem = ((uint32_t)A.d[0] + 2u * A.r) & 31u;
    return ~w & ((xw == A.wh - 1u && rem) ? (1u << rem) - 1u : 0xFFFFFFFFu);
}

// x sweep: the squared distance along halo row `row` from halo voxel hx (R <= hx < R + dims[0]) to the nearest target
// within R, FAR when there is none
__host__ __device__ inline uint32_t dist_x(const DistArgs& A, uint64_t row, uint32_t hx)
{
    const uint32_t w = hx >> 5, b = hx & 31u;
    const uint32_t here = dist_targets(A, row, w);
    uint32_t best = kDistFar;
    uint32_t m = here & (0xFFFFFFFFu >> (31u - b));  // at or below hx
    uint32_t k = w;
    const uint32_t wlo = (hx - A.r) >> 5, whi = (hx + A.r) >> 5;  // hx + R is a voxel of the halo row
    while (!m && k > wlo)
        m = dist_targets(A, row, --k);
    if (m)
        best = hx - (32u * k + 31u - (uint32_t)__builtin_clz(m));
    m = here & (0xFFFFFFFFu << b);  // at or above hx
    k = w;
    while (!m && k < whi)
        m = dist_targets(A, row, ++k);
    if (m) {
        const uint32_t up = 32u * k + (uint32_t)__builtin_ctz(m) - hx;
        best = up < best ? up : best;
    }
    return best <= A.r ? best * best : kDistFar;
}

// ---- the scan of one output ---------------------------------------------------------------------------------------------

// min over |k| <= R of slab[c + k][lane] + k^2 for centre row c of a slab of 64-lane rows (c - R and c + R are rows of the
// slab), FAR above R^2.  Runs outwards from k = 0 and stops when k^2 >= the best so far: a row further out adds k^2 or more.
__host__ __device__ inline uint32_t dist_scan(const DistArgs& A, const uint16_t* slab, uint32_t c, uint32_t lane)
{
    VXRT_DIST_CHECK(kDistSlab, c * kDistTile + lane);
    uint32_t best = slab[c * kDistTile + lane];
    for (uint32_t k = 1; k <= A.r && k * k < best; ++k) {
        VXRT_DIST_CHECK(kDistSlab, (c - k) * kDistTile + lane);
        VXRT_DIST_CHECK(kDistSlab, (c + k) * kDistTile + lane);
        const uint32_t a = slab[(c - k) * kDistTile + lane], b = slab[(c + k) * kDistTile + lane];
        const uint32_t v = (a < b ? a : b) + k * k;
        best = v < best ? v : best;
    }
    return best > A.r2 ? kDistFar : best;
}

// ---- empty-space skip ---------------------------------------------------------------------------------------------------

// occupancy cell (xw, cy, cz) of the halo: some target in the word's 8 rows x 8 slices
__host__ __device__ inline void dist_occ_cell(const DistArgs& A, uint32_t xw, uint32_t cy, uint32_t cz)
{
    uint32_t any = 0u;
    for (uint32_t z = cz * kDistCell; z < (cz + 1u) * kDistCell && z < A.hz; ++z)
        for (uint32_t y = cy * kDistCell; y < (cy + 1u) * kDistCell && y < A.hy; ++y)
            any |= dist_targets(A, (uint64_t)y + (uint64_t)A.hy * z, xw);
    const uint64_t i = (uint64_t)xw + (uint64_t)A.wh * ((uint64_t)cy + (uint64_t)A.ncy * cz);
    VXRT_DIST_CHECK(kDistOcc, i);
    A.occ[i] = any ? 1 : 0;
}

// the share `part` of `parts` of tile t's halo neighbourhood (the tile grown by R: halo voxels 64 t .. 64 t + 63 + 2R per
// axis, cut to the halo) holds an occupied cell
__host__ __device__ inline bool dist_tile_part(const DistArgs& A, uint32_t t, uint32_t part, uint32_t parts)
{
    const uint32_t tx = t % A.ntx, tr = t / A.ntx, ty = tr % A.nty, tz = tr / A.nty;
    const uint32_t span = kDistTile + 2u * A.r - 1u;
    const uint32_t xa = (tx * kDistTile) >> 5, ya = (ty * kDistTile) / kDistCell, za = (tz * kDistTile) / kDistCell;
    uint32_t xb = (tx * kDistTile + span) >> 5, yb = (ty * kDistTile + span) / kDistCell, zb = (tz * kDistTile + span) / kDistCell;
    xb = xb < A.wh - 1u ? xb : A.wh - 1u;
    yb = yb < A.ncy - 1u ? yb : A.ncy - 1u;
    zb = zb < A.ncz - 1u ? zb : A.ncz - 1u;
    const uint32_t nx = xb - xa + 1u, ny = yb - ya + 1u, n = nx * ny * (zb - za + 1u);  // at most 19 * 73 * 73
    for (uint32_t i = part; i < n; i += parts) {
        const uint32_t x = xa + i % nx, q = i / nx, y = ya + q % ny, z = za + q / ny;
        const uint64_t c = (uint64_t)x + (uint64_t)A.wh * ((uint64_t)y + (uint64_t)A.ncy * z);
        VXRT_DIST_CHECK(kDistOcc, c);
        if (A.occ[c])
            return true;
    }
    return false;
}

__host__ __device__ inline void dist_tile_store(const DistArgs& A, uint32_t t, bool any)
{
    VXRT_DIST_CHECK(kDistLive, t);
    A.live[t] = (any || !A.skip) ? 1 : 0;
}

// some live tile (tx, ty, *) reads slice hz of g2: tile tz reads the slices 64 tz .. 64 tz + 63 + 2R
__host__ __device__ inline bool dist_slice_live(const DistArgs& A, uint32_t tx, uint32_t ty, uint32_t hz)
{
    const uint32_t span = kDistTile + 2u * A.r - 1u;
    uint32_t tz = hz > span ? (hz - span + kDistTile - 1u) / kDistTile : 0u;
    for (; tz < A.ntz && tz * kDistTile <= hz; ++tz) {
        const uint32_t t = tx + A.ntx * (ty + A.nty * tz);
        VXRT_DIST_CHECK(kDistLive, t);
        if (A.live[t])
            return true;
    }
    return false;
}

// ---- y sweep: workgroup (tx, ty, hz), a slab of min(64 + 2R, hy - 64 ty) rows of x distances --------------------------------

// slab row r, lane: the x distance of voxel x = 64 tx + lane in halo row (64 ty + r, hz)
__host__ __device__ inline void dist_y_load(const DistArgs& A, uint16_t* slab, uint32_t tx, uint32_t ty, uint32_t hz, uint32_t r,
                                            uint32_t lane)
{
    const uint32_t x = tx * kDistTile + lane;
    uint32_t v = kDistFar;
    if (x < (uint32_t)A.d[0])
        v = dist_x(A, (uint64_t)(ty * kDistTile + r) + (uint64_t)A.hy * hz, x + A.r);
    VXRT_DIST_CHECK(kDistSlab, r * kDistTile + lane);
    slab[r * kDistTile + lane] = (uint16_t)v;
}

// output j of the slab (row y = 64 ty + j < dims[1] of B), lane
__host__ __device__ inline void dist_y_store(const DistArgs& A, const uint16_t* slab, uint32_t tx, uint32_t ty, uint32_t hz,
                                             uint32_t j, uint32_t lane)
{
    const uint32_t x = tx * kDistTile + lane, y = ty * kDistTile + j;
    if (x >= (uint32_t)A.d[0])
        return;
    const uint64_t i = (uint64_t)x + (uint64_t)A.d[0] * ((uint64_t)y + (uint64_t)A.d[1] * hz);
    VXRT_DIST_CHECK(kDistG2, i);
    A.g2[i] = (uint16_t)dist_scan(A, slab, j + A.r, lane);
}

// ---- z sweep: workgroup (tx, rows y0 .. y0 + 7, tz), per row a slab of min(64 + 2R, hz - 64 tz) slices of g2 ------------------

__host__ __device__ inline void dist_z_load(const DistArgs& A, uint16_t* slab, uint32_t tx, uint32_t y, uint32_t tz, uint32_t r,
                                            uint32_t lane)
{
    const uint32_t x = tx * kDistTile + lane;
    uint32_t v = kDistFar;
    if (x < (uint32_t)A.d[0]) {
        const uint64_t i = (uint64_t)x + (uint64_t)A.d[0] * ((uint64_t)y + (uint64_t)A.d[1] * (uint64_t)(tz * kDistTile + r));
        VXRT_DIST_CHECK(kDistG2, i);
        v = A.g2[i];
    }
    VXRT_DIST_CHECK(kDistSlab, r * kDistTile + lane);
    slab[r * kDistTile + lane] = (uint16_t)v;
}

// The tally of one workgroup: zero, near, far, max_d2 and the sum of the values that are not FAR.  A workgroup adds at
// most 8 x 64 x 64 values of at most 65025, so the sum fits 32 bits until it joins the summary's 64.
struct DistTally {
    uint32_t zero, near, far, max_d2, sum;
};

__host__ __device__ inline void dist_tally(DistTally& t, uint32_t v)
{
    const bool far = v == kDistFar;
    t.far += far ? 1u : 0u;
    t.near += !far && v ? 1u : 0u;
    t.zero += v ? 0u : 1u;
    t.max_d2 = !far && v > t.max_d2 ? v : t.max_d2;
    t.sum += far ? 0u : v;
}

// output j of the slab (slice z = 64 tz + j < dims[2] of B), lane, or FAR without a slab for a tile that is not live
__host__ __device__ inline void dist_z_store(const DistArgs& A, const uint16_t* slab, uint32_t tx, uint32_t y, uint32_t tz,
                                             uint32_t j, uint32_t lane, DistTally& t)
{
    const uint32_t x = tx * kDistTile + lane, z = tz * kDistTile + j;
    if (x >= (uint32_t)A.d[0])
        return;
    const uint32_t v = slab ? dist_scan(A, slab, j + A.r, lane) : kDistFar;
    const uint64_t i = (uint64_t)x + (uint64_t)A.d[0] * ((uint64_t)y + (uint64_t)A.d[1] * z);
    VXRT_DIST_CHECK(kDistOut, i);
    A.out[i] = (uint16_t)v;
    dist_tally(t, v);
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_dist.hip on the box o, d
hipError_t distance_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t radius, uint32_t mode, void* work,
                          uint16_t* dist2, vxrt_distance_summary* summary, hipStream_t stream);
#endif

}  // namespace vxrt
