// vxrt_surface.hpp -- surface extraction (include/vxrt.h, vxrt_extract_surface): the pieces shared by the kernels of
// vxrt_surface.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/surface_check.cpp, through
// tests/tools/hoststub): the workspace layout, the face words and face bits of the halo, the walk over one row of a mask
// (counting its quads, or writing them), the test for an identical run in another row and the records a quad writes.
//
// Halo.  The box B grown by one voxel on every side: halo voxel (hx, hy, hz) is world voxel origin - 1 + (hx, hy, hz), so
// voxel (x, y, z) of B is halo voxel (x + 1, y + 1, z + 1).  Its bits come from k_read_region (outside the world: 0).  A
// row of the halo is wh words; bits 1 .. dims[0] of a row are voxels of B, bit 0 and bit dims[0] + 1 the x neighbours.
// Neighbours.  VXRT_SURF_OPEN reads a neighbour outside B from the halo; VXRT_SURF_CAP reads it as empty.
// Rows.  A row is (d, s, v): direction, slice, row of the slice's mask.  Row index, the canonical order of the output:
//   d = 0, 1 (-x, +x)   s = x, v = z, u = y:   d * dims[0] * dims[2] + x * dims[2] + z
//   d = 2, 3 (-y, +y)   s = y, v = z, u = x:   nrx + (d - 2) * dims[1] * dims[2] + y * dims[2] + z
//   d = 4, 5 (-z, +z)   s = z, v = y, u = x:   nrx + (d - 2) * dims[1] * dims[2] + z * dims[1] + y
// with nrx = 2 * dims[0] * dims[2].  The count pass leaves one count per row, the scan turns it into the index of the
// row's first quad, the emit pass walks the row again and writes.
// Runs along x (d >= 2) are found in the face words S & ~N of the row: the starts of a word by one shift with the carry of
// the word below, the end of a run by a count of trailing zeros, the identical run of another row by comparing the words
// under the run grown by one bit on each side.  Runs along y (d < 2) are walked bit by bit by the lane that owns x.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into an array of the workspace or the outputs against
// that array's size (array: one of the kSurf* ids below).  The kernels leave it empty.
#ifndef VXRT_SURF_CHECK
#define VXRT_SURF_CHECK(array, index)
#endif

namespace vxrt {

constexpr int32_t kSurfMaxDim = 1024;
constexpr uint64_t kSurfMaxVoxels = 1ull << 28;
constexpr uint32_t kSurfGroup = 256;           // rows per workgroup of the scan
constexpr uint32_t kSurfMaxIndexed = 1u << 30;  // quads whose vertex indices 4 i + 3 fit uint32
enum { kSurfHalo, kSurfCounts, kSurfGroups, kSurfQuads, kSurfVerts, kSurfTris, kSurfArrays };
// summary words (vxrt_surface_summary)
enum { kSurfSumSolid, kSurfSumFaces, kSurfSumQuads, kSurfSumWritten, kSurfSumFacesDir, kSurfSumQuadsDir = kSurfSumFacesDir + 6 };

// the workspace: sections of bytes, each on a 256-byte boundary (include/vxrt.h states the same formula)
struct SurfLayout : HaloBox {       // the halo box (vxrt_region.hpp): B grown by 1
    uint64_t halo, counts, groups;  // byte offsets
    uint64_t total_bytes;
    uint32_t nrx, nryz, nrows;   // rows of the x directions, of the y and z directions, all
    uint32_t ngroups;
};

// false outside the contract (L.fault: why): the dims and, when `o` is given, the halo box within int32
inline bool surf_layout(const int32_t* o, const int32_t d[3], SurfLayout& L)
{
    const bool wide = d[0] > kSurfMaxDim || d[1] > kSurfMaxDim || d[2] > kSurfMaxDim;
    L.fault = wide ? kBoxDims : halo_box(o, d, 1, kSurfMaxVoxels, L);
    if (L.fault != kBoxOk)
        return false;
    L.nrx = 2u * (uint32_t)d[0] * (uint32_t)d[2];
    L.nryz = 4u * (uint32_t)d[1] * (uint32_t)d[2];
    L.nrows = L.nrx + L.nryz;
    L.ngroups = (L.nrows + kSurfGroup - 1u) / kSurfGroup;
    Sections S;
    L.halo = S.take(4u * L.nhalo);
    L.counts = S.take(4u * (uint64_t)L.nrows);
    L.groups = S.take(4u * (uint64_t)L.ngroups);
    L.total_bytes = S.at;
    return true;
}

// what the surface kernels read and write (device pointers; host pointers in the harness)
struct SurfArgs {
    const uint32_t* halo;  // the halo's region words (k_read_region)
    uint32_t* counts;      // per row: its quads, then (after the scan) the quads before it within its group of 256 rows
    uint32_t* groups;      // per group: its quads, then the quads before it
    uint32_t* quads;       // output: vxrt_quad records, two words each (may be NULL when capacity is 0)
    int32_t* verts;        // output: 12 int32 per quad, or NULL
    uint32_t* tris;        // output: 6 uint32 per quad, or NULL
    uint32_t* summary;     // output: vxrt_surface_summary
    int32_t d[3];
    uint32_t open, capacity;  // capacity: quads that may be written
    uint32_t wh, hy, nrx, nryz, nrows, ngroups;
};

inline void surf_args(SurfArgs& A, const SurfLayout& L, const int32_t d[3], uint32_t mode, void* work, uint32_t* quads,
                      uint32_t capacity, int32_t* verts, uint32_t* tris, uint32_t* summary)
{
    A.halo = (const uint32_t*)((char*)work + L.halo);
    A.counts = (uint32_t*)((char*)work + L.counts);
    A.groups = (uint32_t*)((char*)work + L.groups);
    A.quads = quads;
    A.verts = verts;
    A.tris = tris;
    A.summary = summary;
    for (int k = 0; k < 3; ++k)
        A.d[k] = d[k];
    A.open = mode;
    A.capacity = verts && capacity > kSurfMaxIndexed ? kSurfMaxIndexed : capacity;
    A.wh = L.wh;
    A.hy = L.hy;
    A.nrx = L.nrx;
    A.nryz = L.nryz;
    A.nrows = L.nrows;
    A.ngroups = L.ngroups;
}

// The tally of one lane: solid voxels, faces and quads by direction.  A lane counts in one direction only.
struct SurfTally {
    uint32_t solid, faces, quads;
};

// ---- the halo ------------------------------------------------------------------------------------------------------------

// word k of the halo row of B's row (y, z), -1 <= y <= dims[1], -1 <= z <= dims[2]
__host__ __device__ inline uint32_t surf_halo(const SurfArgs& A, int32_t y, int32_t z, uint32_t k)
{
    const uint64_t i = ((uint64_t)(uint32_t)(y + 1) + (uint64_t)A.hy * (uint32_t)(z + 1)) * A.wh + k;
    VXRT_SURF_CHECK(kSurfHalo, i);
    return A.halo[i];
}

// the bits of halo word k that are voxels of B: halo bits 1 .. dims[0]
__host__ __device__ inline uint32_t surf_xmask(const SurfArgs& A, uint32_t k)
{
    const int32_t a = k ? 0 : 1, b = A.d[0] - 32 * (int32_t)k;  // the last voxel of B is bit dims[0] of the row
    return b < a ? 0u : bit_range(a, b > 31 ? 31 : b);
}

// word k of the faces of direction d (2 .. 5) in row v of slice s: solid in B, the neighbour across the face empty
__host__ __device__ inline uint32_t surf_face_word(const SurfArgs& A, uint32_t d, int32_t s, int32_t v, uint32_t k)
{
    const int32_t y = d < 4u ? s : v, z = d < 4u ? v : s, step = (d & 1u) ? 1 : -1;
    const int32_t ny = d < 4u ? y + step : y, nz = d < 4u ? z : z + step;
    const uint32_t solid = surf_halo(A, y, z, k) & surf_xmask(A, k);
    if (!solid || (!A.open && (ny < 0 || ny >= A.d[1] || nz < 0 || nz >= A.d[2])))
        return solid;
    return solid & ~surf_halo(A, ny, nz, k);
}

// the face of direction d (0 or 1) of voxel (x, y, z) of B
__host__ __device__ inline uint32_t surf_face_bit(const SurfArgs& A, uint32_t d, int32_t x, int32_t y, int32_t z)
{
    const uint32_t hx = (uint32_t)x + 1u, hn = d ? hx + 1u : hx - 1u;
    const uint32_t w = surf_halo(A, y, z, hx >> 5);
    if (!((w >> (hx & 31u)) & 1u))
        return 0u;
    if (!A.open && (d ? x == A.d[0] - 1 : x == 0))
        return 1u;
    const uint32_t wn = (hn >> 5) == (hx >> 5) ? w : surf_halo(A, y, z, hn >> 5);
    return ~(wn >> (hn & 31u)) & 1u;
}

// ---- a quad's records ---------------------------------------------------------------------------------------------------

// quad `pos`: direction d, slice s, lowest in-plane voxel (u, v), extent (w, h)
__host__ __device__ inline void surf_write(const SurfArgs& A, uint32_t pos, uint32_t d, uint32_t s, uint32_t u, uint32_t v,
                                           uint32_t w, uint32_t h)
{
    const uint32_t a = d >> 1;
    const uint32_t x = a == 0u ? s : u, y = a == 0u ? u : (a == 1u ? s : v), z = a == 2u ? s : v;
    VXRT_SURF_CHECK(kSurfQuads, 2u * (uint64_t)pos + 1u);
    A.quads[2u * (uint64_t)pos] = x | y << 10 | z << 20;
    A.quads[2u * (uint64_t)pos + 1u] = (w - 1u) | (h - 1u) << 10 | d << 20;
    if (!A.verts)
        return;
    // the corners (u, v), (u + w, v), (u + w, v + h), (u, v + h) on the plane 256 (s + (d & 1)): 48 contiguous bytes
    const int32_t p = 256 * (int32_t)(s + (d & 1u)), u0 = 256 * (int32_t)u, u1 = 256 * (int32_t)(u + w), v0 = 256 * (int32_t)v,
                  v1 = 256 * (int32_t)(v + h);
    int32_t* q = A.verts + 12u * (uint64_t)pos;
    VXRT_SURF_CHECK(kSurfVerts, 12u * (uint64_t)pos + 11u);
    for (int c = 0; c < 4; ++c) {
        const int32_t cu = (c == 1 || c == 2) ? u1 : u0, cv = c >= 2 ? v1 : v0;
        q[3 * c + 0] = a == 0u ? p : cu;
        q[3 * c + 1] = a == 0u ? cu : (a == 1u ? p : cv);
        q[3 * c + 2] = a == 2u ? p : cv;
    }
    // e_u x e_v is +x, -y, +z: the corner order as it is faces +x, -y, +z, and is reversed for the other three
    const bool flip = ((d & 1u) != 0u) == (a == 1u);
    const uint32_t b = 4u * pos;
    uint32_t* t = A.tris + 6u * (uint64_t)pos;
    VXRT_SURF_CHECK(kSurfTris, 6u * (uint64_t)pos + 5u);
    t[0] = b;
    t[1] = flip ? b + 2u : b + 1u;
    t[2] = flip ? b + 1u : b + 2u;
    t[3] = b;
    t[4] = flip ? b + 3u : b + 2u;
    t[5] = flip ? b + 2u : b + 3u;
}

// ---- rows of the y and z directions: runs along x, in halo bits ------------------------------------------------------------

// row v of slice s has exactly the run [u, e) (halo bits; bits u - 1 and e are bits of the row): under the run grown by
// one bit on each side the face words hold the run and nothing else
__host__ __device__ inline bool surf_same_yz(const SurfArgs& A, uint32_t d, int32_t s, int32_t v, uint32_t u, uint32_t e)
{
    for (uint32_t k = (u - 1u) >> 5; k <= e >> 5; ++k) {
        const uint32_t lo = u - 1u > 32u * k ? u - 1u - 32u * k : 0u, hi = e < 32u * k + 31u ? e - 32u * k : 31u;
        uint32_t want = bit_range((int)lo, (int)hi);
        const uint32_t m = want;
        if (u - 1u >= 32u * k)
            want &= ~(1u << lo);
        if (e <= 32u * k + 31u)
            want &= ~(1u << hi);
        if ((surf_face_word(A, d, s, v, k) & m) != want)
            return false;
    }
    return true;
}

// Row j (0 .. nryz - 1) of the y and z directions.  kEmit false: returns the row's quads and tallies its faces (and, once
// per row of B, its solid voxels).  kEmit true: writes the row's quads from index `pos` on, up to the capacity.
template <bool kEmit>
__host__ __device__ inline uint32_t surf_row_yz(const SurfArgs& A, uint32_t j, uint32_t pos, SurfTally& t, uint32_t& dir)
{
    const uint32_t plane = (uint32_t)A.d[1] * (uint32_t)A.d[2], d = 2u + j / plane, r = j % plane;
    const uint32_t nv = d < 4u ? (uint32_t)A.d[2] : (uint32_t)A.d[1];
    const int32_t s = (int32_t)(r / nv), v = (int32_t)(r % nv);
    dir = d;
    uint32_t n = 0u, carry = 0u;
    for (uint32_t k = 0; k < A.wh; ++k) {
        const uint32_t f = surf_face_word(A, d, s, v, k);
        if (!kEmit) {
            t.faces += (uint32_t)__builtin_popcount(f);
            if (d == 2u)
                t.solid += (uint32_t)__builtin_popcount(surf_halo(A, s, v, k) & surf_xmask(A, k));
        }
        uint32_t st = f & ~(f << 1 | carry);
        carry = f >> 31;
        while (st) {
            const uint32_t b = (uint32_t)__builtin_ctz(st), u = 32u * k + b;
            st &= st - 1u;
            // the run's end: the first clear bit above u (bit dims[0] + 1 of the row is clear)
            uint32_t kk = k, z = ~f & (0xFFFFFFFFu << b);
            while (!z)
                z = ~surf_face_word(A, d, s, v, ++kk);
            const uint32_t e = 32u * kk + (uint32_t)__builtin_ctz(z);
            if (v > 0 && surf_same_yz(A, d, s, v - 1, u, e))
                continue;  // the quad started in a row above
            if (kEmit) {
                if (pos >= A.capacity)
                    return n;
                uint32_t h = 1u;
                while ((uint32_t)v + h < nv && surf_same_yz(A, d, s, v + (int32_t)h, u, e))
                    ++h;
                surf_write(A, pos++, d, (uint32_t)s, u - 1u, (uint32_t)v, e - u, h);
            }
            ++n;
        }
    }
    t.quads += n;
    return n;
}

// ---- rows of the x directions: runs along y, one face bit at a time --------------------------------------------------------

// row z of slice x has exactly the run [u, e) of y
__host__ __device__ inline bool surf_same_x(const SurfArgs& A, uint32_t d, int32_t x, int32_t z, int32_t u, int32_t e)
{
    if (u > 0 && surf_face_bit(A, d, x, u - 1, z))
        return false;
    if (e < A.d[1] && surf_face_bit(A, d, x, e, z))
        return false;
    for (int32_t y = u; y < e; ++y)
        if (!surf_face_bit(A, d, x, y, z))
            return false;
    return true;
}

// Row (d, x, z) of the x directions, as surf_row_yz.  The walk over y carries the open run of row z and whether row z - 1
// has matched it so far: a start where the row above starts too, set bits under set bits, an end under an end.
template <bool kEmit>
__host__ __device__ inline uint32_t surf_row_x(const SurfArgs& A, uint32_t d, int32_t x, int32_t z, uint32_t pos, SurfTally& t)
{
    uint32_t n = 0u, above = 0u;  // above: the face bit of row z - 1 at y - 1
    bool run = false, same = false;
    int32_t u = 0;
    for (int32_t y = 0; y <= A.d[1]; ++y) {
        const uint32_t c = y < A.d[1] ? surf_face_bit(A, d, x, y, z) : 0u;
        const uint32_t p = y < A.d[1] && z > 0 ? surf_face_bit(A, d, x, y, z - 1) : 0u;
        if (c && !run) {
            run = true;
            u = y;
            same = !above && p;
        } else if (c) {
            same = same && p;
        } else if (run) {
            run = false;
            if (!(same && !p)) {
                if (kEmit) {
                    if (pos >= A.capacity)
                        return n;
                    uint32_t h = 1u;
                    while (z + (int32_t)h < A.d[2] && surf_same_x(A, d, x, z + (int32_t)h, u, y))
                        ++h;
                    surf_write(A, pos++, d, (uint32_t)x, (uint32_t)u, (uint32_t)z, (uint32_t)(y - u), h);
                }
                ++n;
            }
        }
        above = p;
        if (!kEmit)
            t.faces += c;
    }
    t.quads += n;
    return n;
}

// the index of row (d, x, z) of the x directions in the counts
__host__ __device__ inline uint32_t surf_row_index_x(const SurfArgs& A, uint32_t d, int32_t x, int32_t z)
{
    return (d * (uint32_t)A.d[0] + (uint32_t)x) * (uint32_t)A.d[2] + (uint32_t)z;
}

// the index of the first quad of row i after the scan
__host__ __device__ inline uint32_t surf_row_start(const SurfArgs& A, uint32_t i)
{
    VXRT_SURF_CHECK(kSurfCounts, i);
    VXRT_SURF_CHECK(kSurfGroups, i / kSurfGroup);
    return A.counts[i] + A.groups[i / kSurfGroup];
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_surface.hip on the box o, d
hipError_t extract_surface(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t mode, void* work, vxrt_quad* quads,
                           uint32_t capacity, int32_t* verts, uint32_t* tris, vxrt_surface_summary* summary, hipStream_t stream);
#endif

}  // namespace vxrt
