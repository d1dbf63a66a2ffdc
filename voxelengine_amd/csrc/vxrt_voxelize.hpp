// vxrt_voxelize.hpp -- triangle meshes into region-layout bits (include/vxrt.h, vxrt_voxelize_mesh): the pieces shared by
// the kernels of vxrt_voxelize.hip, the host side in vxrt_api_query.hip and the host harness of the tests
// (tests/tools/voxelize_check.cpp, through tests/tools/hoststub): the workspace layout, a triangle's validity, clipped
// voxel boxes and work items, the integer separating-axis test, the three levels of the surface cull, the solid toggle of
// one column, the item lookup and the last pass (suffix XOR along a row, the OR of the fields, the popcounts).
//
// Arithmetic.  Coordinates are fixed point, 256 units per voxel, every coordinate a triangle uses in [-2^18, 2^18] and
// every voxel of the region below 1024 * 256 = 2^18.  So an edge component is at most 2^19 in magnitude, a normal component
// (a difference of two products of edge components) at most 2^39, a box's doubled centre at most 2^19 and its doubled half
// size at most 2^18; a vertex relative to a doubled centre is at most 2^20.  Every product below is int32 x int32 -> int64
// (edge function terms, at most 2^39) or int64 x int32 (plane terms, at most 2^39 * 2^20 = 2^59); a plane value is a sum of
// three such terms and stays below 2^61 + 2^60 < 2^62.  Nothing overflows int64; the harness is built with -ftrapv.
//
// Work.  One lane per triangle (vox_setup_lane) classifies it and counts its work items: a surface item is 64 blocks of
// 64 x 8 x 8 voxels of the triangle's clipped voxel box, a solid item 64 columns (j, k) of the yz box of the voxel centres
// the triangle can cover.  The counts are scanned (per group of 256 triangles, then over the groups), and waves take items
// from one ticket counter until it passes the total; the host never reads a count.
//   surface item: lane = block, the separating-axis test against the block's box (cut to the triangle's voxel box), a
//     ballot; per surviving block lane = one of its 64 rows, the same test against the row's box, a ballot; per surviving
//     row lane = voxel along x, the test against the voxel's cube, and the ballot is the row's 64 bits: at most two atomic
//     ORs into the output.  The test against a box is exact for the box, so a culled block or row holds no set voxel.
//   solid item: lane = column; the top-left rule on the yz projection, then one floor division gives m, the number of
//     voxels of the row whose centre lies before the plane, and one atomic XOR toggles bit m - 1 of the row.
//   last pass: the suffix XOR of every toggle row (voxel i is set when an odd number of toggles lie at or above i), ORed
//     with the surface bits, and the summary's popcounts.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into the mesh, the workspace or the outputs against that
// array's size (array: one of the kVox* ids below).  The kernels leave it empty.
#ifndef VXRT_VOX_CHECK
#define VXRT_VOX_CHECK(array, index)
#endif
// The harness counts the ballots of each level of the surface cull with this (level 0: blocks, 1: rows, 2: voxels).
#ifndef VXRT_VOX_COUNT
#define VXRT_VOX_COUNT(level)
#endif
// The harness makes this a run-time switch, to compare against a run in which every block and row descends.
#ifndef VXRT_VOX_CULL
#define VXRT_VOX_CULL true
#endif

namespace vxrt {

constexpr int32_t kVoxUnit = 256, kVoxMaxDim = 1024, kVoxMaxCoord = 1 << 18;
constexpr uint32_t kVoxMaxTriangles = 1u << 24;
constexpr uint32_t kVoxSurface = 1u, kVoxSolid = 2u;
constexpr uint32_t kVoxGroup = 256;  // triangles of one setup workgroup: the unit of the first scan
constexpr uint32_t kVoxInvalid = 1u, kVoxDegenerate = 2u, kVoxOutside = 4u;
enum { kVoxVerts, kVoxTris, kVoxToggle, kVoxTriPrefix, kVoxGroupPrefix, kVoxBits };
// summary words (vxrt_voxelize_summary)
enum { kVoxSumSet, kVoxSumSurface, kVoxSumSolid, kVoxSumTriangles, kVoxSumInvalid, kVoxSumDegenerate, kVoxSumOutside, kVoxSumReserved };
// counter section of the workspace, uint64 each
enum { kVoxTicket, kVoxTotal };

// the workspace: sections of bytes, each on a 256-byte boundary (include/vxrt.h states the same formula)
struct VoxLayout {
    uint64_t toggle, tri_prefix, group_prefix, counters;  // byte offsets
    uint64_t total_bytes;
    uint64_t words;  // region words of the output
    uint32_t wpr, ngroups;
};

// false outside the contract on dims and n_triangles
inline bool vox_layout(const int32_t d[3], uint64_t n_triangles, VoxLayout& L)
{
    if (n_triangles > kVoxMaxTriangles)
        return false;
    for (int k = 0; k < 3; ++k)
        if (d[k] < 1 || d[k] > kVoxMaxDim)
            return false;
    L.wpr = (uint32_t)region_words_per_row(d[0]);
    L.words = (uint64_t)L.wpr * (uint64_t)d[1] * (uint64_t)d[2];
    L.ngroups = (uint32_t)((n_triangles + kVoxGroup - 1u) / kVoxGroup);
    Sections S;
    L.toggle = S.take(4u * L.words);
    L.tri_prefix = S.take(4u * n_triangles);
    L.group_prefix = S.take(8u * (uint64_t)L.ngroups);
    L.counters = S.take(256u);
    L.total_bytes = S.at;
    return true;
}

// what the kernels read and write (device pointers; host pointers in the harness)
struct VoxArgs {
    const int32_t* verts;    // 3 per vertex
    const uint32_t* tris;    // 3 per triangle
    uint32_t* toggle;        // region layout: the solid field's toggles, then (in place) nothing else
    uint32_t* tri_prefix;    // per triangle: items of the triangles before it in its group
    uint64_t* group_prefix;  // per group: its items (after setup), then the items of the groups before it (after the scan)
    uint64_t* counters;      // kVoxTicket, kVoxTotal
    uint32_t* bits;          // output: the surface bits, then the whole field
    uint32_t* summary;       // output: vxrt_voxelize_summary
    uint32_t nv, nt, modes;
    uint32_t wpr, ngroups;
    int32_t d[3];
};

inline void vox_args(VoxArgs& A, const VoxLayout& L, const int32_t* verts, uint32_t nv, const uint32_t* tris, uint32_t nt,
                     const int32_t d[3], uint32_t modes, void* work, uint32_t* bits, uint32_t* summary)
{
    A.verts = verts;
    A.tris = tris;
    A.toggle = (uint32_t*)((char*)work + L.toggle);
    A.tri_prefix = (uint32_t*)((char*)work + L.tri_prefix);
    A.group_prefix = (uint64_t*)((char*)work + L.group_prefix);
    A.counters = (uint64_t*)((char*)work + L.counters);
    A.bits = bits;
    A.summary = summary;
    A.nv = nv;
    A.nt = nt;
    A.modes = modes;
    A.wpr = L.wpr;
    A.ngroups = L.ngroups;
    for (int k = 0; k < 3; ++k)
        A.d[k] = d[k];
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline uint32_t vox_atom_xor(uint32_t* p, uint32_t v) { return atomicXor(p, v); }
#else
inline uint32_t vox_atom_xor(uint32_t* p, uint32_t v)
{
    const uint32_t o = *p;
    *p = o ^ v;
    return o;
}
#endif

// ---- a triangle ---------------------------------------------------------------------------------------------------------

struct VoxTri {
    int32_t v[3][3];
    int64_t n[3];            // (v1 - v0) x (v2 - v0): at most 2^39 per component
    int32_t mn[3], mx[3];    // the vertices' bounding box, units
    int32_t lo[3], hi[3];    // voxels whose closed cube meets the closed bounding box, cut to the region, inclusive
    int32_t clo[2], chi[2];  // rows j and slices k whose centre lies in the bounding box's y and z ranges, cut to the region
};

// loads triangle t; returns its kVox* flags.  An invalid triangle loads no vertex past the first bad index or coordinate.
__host__ __device__ inline uint32_t vox_tri_load(const VoxArgs& A, uint32_t t, VoxTri& T)
{
    uint32_t idx[3];
    for (int i = 0; i < 3; ++i) {
        VXRT_VOX_CHECK(kVoxTris, 3ull * t + i);
        idx[i] = A.tris[3ull * t + i];
        if (idx[i] >= A.nv)
            return kVoxInvalid;
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            VXRT_VOX_CHECK(kVoxVerts, 3ull * idx[i] + k);
            const int32_t c = A.verts[3ull * idx[i] + k];
            if (c < -kVoxMaxCoord || c > kVoxMaxCoord)
                return kVoxInvalid;
            T.v[i][k] = c;
        }
    int32_t e[3], g[3];  // at most 2^19
    for (int k = 0; k < 3; ++k) {
        e[k] = T.v[1][k] - T.v[0][k];
        g[k] = T.v[2][k] - T.v[0][k];
    }
    T.n[0] = (int64_t)e[1] * g[2] - (int64_t)e[2] * g[1];
    T.n[1] = (int64_t)e[2] * g[0] - (int64_t)e[0] * g[2];
    T.n[2] = (int64_t)e[0] * g[1] - (int64_t)e[1] * g[0];
    uint32_t flags = (T.n[0] | T.n[1] | T.n[2]) ? 0u : kVoxDegenerate;
    for (int k = 0; k < 3; ++k) {
        const int32_t a = T.v[0][k], b = T.v[1][k], c = T.v[2][k];
        T.mn[k] = a < b ? (a < c ? a : c) : (b < c ? b : c);
        T.mx[k] = a > b ? (a > c ? a : c) : (b > c ? b : c);
        if (T.mx[k] < 0 || T.mn[k] > kVoxUnit * A.d[k])
            flags |= kVoxOutside;
        // cube i = [256 i, 256 (i + 1)] meets [mn, mx] when 256 i <= mx and mn <= 256 (i + 1); >> floors
        const int32_t lo = (T.mn[k] - 1) >> 8, hi = T.mx[k] >> 8;
        T.lo[k] = lo < 0 ? 0 : lo;
        T.hi[k] = hi > A.d[k] - 1 ? A.d[k] - 1 : hi;
        if (k) {  // centre 256 j + 128 in [mn, mx]
            const int32_t cl = (T.mn[k] + 127) >> 8, ch = (T.mx[k] - 128) >> 8;
            T.clo[k - 1] = cl < 0 ? 0 : cl;
            T.chi[k - 1] = ch > A.d[k] - 1 ? A.d[k] - 1 : ch;
        }
    }
    return flags;
}

// the surface and solid work items of a loaded triangle with flags 0 or kVoxOutside
__host__ __device__ inline void vox_items(const VoxArgs& A, const VoxTri& T, uint32_t& surface, uint32_t& solid)
{
    surface = solid = 0u;
    if ((A.modes & kVoxSurface) && T.lo[0] <= T.hi[0] && T.lo[1] <= T.hi[1] && T.lo[2] <= T.hi[2]) {
        const uint32_t nb = (uint32_t)((T.hi[0] >> 6) - (T.lo[0] >> 6) + 1) * (uint32_t)((T.hi[1] >> 3) - (T.lo[1] >> 3) + 1) *
                            (uint32_t)((T.hi[2] >> 3) - (T.lo[2] >> 3) + 1);  // at most 16 * 128 * 128
        surface = (nb + 63u) >> 6;
    }
    if ((A.modes & kVoxSolid) && T.n[0] != 0 && T.clo[0] <= T.chi[0] && T.clo[1] <= T.chi[1]) {
        const uint32_t nc = (uint32_t)(T.chi[0] - T.clo[0] + 1) * (uint32_t)(T.chi[1] - T.clo[1] + 1);  // at most 2^20
        solid = (nc + 63u) >> 6;
    }
}

// ---- setup: one lane per triangle -----------------------------------------------------------------------------------------

// the flags and the item count of triangle t (0 for an invalid or degenerate one); at most 4096 + 16384
__host__ __device__ inline uint32_t vox_setup_lane(const VoxArgs& A, uint32_t t, uint32_t& flags)
{
    VoxTri T;
    flags = vox_tri_load(A, t, T);
    if (flags & (kVoxInvalid | kVoxDegenerate))
        return 0u;
    uint32_t a, b;
    vox_items(A, T, a, b);
    return a + b;
}

__host__ __device__ inline void vox_setup_store(const VoxArgs& A, uint32_t t, uint32_t before)
{
    VXRT_VOX_CHECK(kVoxTriPrefix, t);
    A.tri_prefix[t] = before;
}

// the (triangle, item of it) of work item `item` < total: the last group, then the last triangle of it, that starts at or
// before the item (a triangle without items shares its start with the next one, so it is never the last)
__host__ __device__ inline void vox_find(const VoxArgs& A, uint64_t item, uint32_t& t, uint32_t& q)
{
    uint32_t lo = 0, hi = A.ngroups - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        VXRT_VOX_CHECK(kVoxGroupPrefix, mid);
        if (A.group_prefix[mid] <= item)
            lo = mid;
        else
            hi = mid - 1u;
    }
    VXRT_VOX_CHECK(kVoxGroupPrefix, lo);
    const uint32_t rest = (uint32_t)(item - A.group_prefix[lo]);
    uint32_t a = lo * kVoxGroup, b = a + kVoxGroup - 1u < A.nt - 1u ? a + kVoxGroup - 1u : A.nt - 1u;
    while (a < b) {
        const uint32_t mid = (a + b + 1u) >> 1;
        VXRT_VOX_CHECK(kVoxTriPrefix, mid);
        if (A.tri_prefix[mid] <= rest)
            a = mid;
        else
            b = mid - 1u;
    }
    VXRT_VOX_CHECK(kVoxTriPrefix, a);
    t = a;
    q = rest - A.tri_prefix[a];
}

// ---- surface: the separating-axis test of a triangle against boxes of voxels ------------------------------------------------

// Per-triangle constants.  A box of voxels lo .. hi (inclusive) has the doubled centre c2 = 256 (lo + hi + 1) and the doubled
// half size h2 = 256 (hi - lo + 1); the vertices are doubled as well, so the test is in whole numbers.  Axis (e, k) is edge
// e crossed with cube axis k: with k1, k2 the other two axes it has the components a[k1] = -edge[k2], a[k2] = edge[k1].
struct VoxSat {
    int64_t n[3], nabs[3], nd;   // the normal, its magnitudes, 2 n . v0 (at most 3 * 2^39 * 2^19)
    int32_t mn2[3], mx2[3];      // the doubled bounding box
    int32_t a[9][2], aabs[9][2]; // at most 2^19
    int64_t pmin[9], pmax[9];    // min and max over the vertices of 2 a . v: at most 2 * 2 * 2^19 * 2^18 = 2^39
};

__host__ __device__ inline void vox_sat_setup(const VoxTri& T, VoxSat& S)
{
    S.nd = 0;
    for (int k = 0; k < 3; ++k) {
        S.n[k] = T.n[k];
        S.nabs[k] = T.n[k] < 0 ? -T.n[k] : T.n[k];
        S.nd += 2 * T.n[k] * T.v[0][k];
        S.mn2[k] = 2 * T.mn[k];
        S.mx2[k] = 2 * T.mx[k];
    }
    for (int e = 0; e < 3; ++e) {
        const int f = e == 2 ? 0 : e + 1;
        const int32_t edge[3] = {T.v[f][0] - T.v[e][0], T.v[f][1] - T.v[e][1], T.v[f][2] - T.v[e][2]};
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * e + k, k1 = k == 2 ? 0 : k + 1, k2 = k1 == 2 ? 0 : k1 + 1;
            const int32_t a1 = -edge[k2], a2 = edge[k1];
            S.a[i][0] = a1;
            S.a[i][1] = a2;
            S.aabs[i][0] = a1 < 0 ? -a1 : a1;
            S.aabs[i][1] = a2 < 0 ? -a2 : a2;
            int64_t mn = 0, mx = 0;
            for (int v = 0; v < 3; ++v) {
                const int64_t p = 2 * ((int64_t)a1 * T.v[v][k1] + (int64_t)a2 * T.v[v][k2]);
                mn = v == 0 || p < mn ? p : mn;
                mx = v == 0 || p > mx ? p : mx;
            }
            S.pmin[i] = mn;
            S.pmax[i] = mx;
        }
    }
}

// the closed triangle meets the closed box of the voxels lo .. hi: no axis of the 13 separates them strictly
__host__ __device__ inline bool vox_sat(const VoxSat& S, const int32_t lo[3], const int32_t hi[3])
{
    int32_t c2[3], h2[3];
    for (int k = 0; k < 3; ++k) {
        c2[k] = kVoxUnit * (lo[k] + hi[k] + 1);
        h2[k] = kVoxUnit * (hi[k] - lo[k] + 1);
        if (S.mn2[k] - c2[k] > h2[k] || S.mx2[k] - c2[k] < -h2[k])
            return false;
    }
    const int64_t val = S.nd - (S.n[0] * c2[0] + S.n[1] * c2[1] + S.n[2] * c2[2]);  // n . (2 v0 - c2)
    const int64_t rn = S.nabs[0] * h2[0] + S.nabs[1] * h2[1] + S.nabs[2] * h2[2];
    if (val > rn || val < -rn)
        return false;
    for (int i = 0; i < 9; ++i) {
        const int k = i % 3, k1 = k == 2 ? 0 : k + 1, k2 = k1 == 2 ? 0 : k1 + 1;
        const int64_t s = (int64_t)S.a[i][0] * c2[k1] + (int64_t)S.a[i][1] * c2[k2];
        const int64_t r = (int64_t)S.aabs[i][0] * h2[k1] + (int64_t)S.aabs[i][1] * h2[k2];
        if (S.pmin[i] - s > r || S.pmax[i] - s < -r)
            return false;
    }
    return true;
}

// block b (in the order x, then y, then z over the blocks the triangle's voxel box meets) as block coordinates
__host__ __device__ inline bool vox_block_coords(const VoxTri& T, uint32_t b, int32_t bc[3])
{
    const uint32_t nx = (uint32_t)((T.hi[0] >> 6) - (T.lo[0] >> 6) + 1), ny = (uint32_t)((T.hi[1] >> 3) - (T.lo[1] >> 3) + 1);
    const uint32_t nz = (uint32_t)((T.hi[2] >> 3) - (T.lo[2] >> 3) + 1);
    if (b >= nx * ny * nz)
        return false;
    bc[0] = (T.lo[0] >> 6) + (int32_t)(b % nx);
    bc[1] = (T.lo[1] >> 3) + (int32_t)(b / nx % ny);
    bc[2] = (T.lo[2] >> 3) + (int32_t)(b / nx / ny);
    return true;
}

// the voxels of block bc, rows y0 .. y1 and slices z0 .. z1 of it, cut to the triangle's voxel box; false when none is left
__host__ __device__ inline bool vox_cut(const VoxTri& T, const int32_t bc[3], int32_t y0, int32_t y1, int32_t z0, int32_t z1,
                                        int32_t lo[3], int32_t hi[3])
{
    lo[0] = 64 * bc[0];
    hi[0] = lo[0] + 63;
    lo[1] = 8 * bc[1] + y0;
    hi[1] = 8 * bc[1] + y1;
    lo[2] = 8 * bc[2] + z0;
    hi[2] = 8 * bc[2] + z1;
    for (int k = 0; k < 3; ++k) {
        lo[k] = lo[k] < T.lo[k] ? T.lo[k] : lo[k];
        hi[k] = hi[k] > T.hi[k] ? T.hi[k] : hi[k];
        if (lo[k] > hi[k])
            return false;
    }
    return true;
}

// level 1, lane = block 64 q + lane of the triangle: the block holds a voxel the triangle may set
__host__ __device__ inline bool vox_block_hit(const VoxArgs& A, const VoxTri& T, const VoxSat& S, uint32_t q, uint32_t lane)
{
    int32_t bc[3], lo[3], hi[3];
    if (!vox_block_coords(T, 64u * q + lane, bc) || !vox_cut(T, bc, 0, 7, 0, 7, lo, hi))
        return false;
    return !(VXRT_VOX_CULL) || vox_sat(S, lo, hi);
}

// level 2, lane = row (lane & 7, lane >> 3) of block bc
__host__ __device__ inline bool vox_row_hit(const VoxArgs& A, const VoxTri& T, const VoxSat& S, const int32_t bc[3], uint32_t lane)
{
    int32_t lo[3], hi[3];
    const int32_t y = (int32_t)(lane & 7u), z = (int32_t)(lane >> 3);
    if (!vox_cut(T, bc, y, y, z, z, lo, hi))
        return false;
    return !(VXRT_VOX_CULL) || vox_sat(S, lo, hi);
}

// level 3, lane = voxel 64 bc[0] + lane of row `row` of block bc: the triangle meets the voxel's cube
__host__ __device__ inline bool vox_voxel_hit(const VoxTri& T, const VoxSat& S, const int32_t bc[3], uint32_t row, uint32_t lane)
{
    const int32_t x = 64 * bc[0] + (int32_t)lane;
    if (x < T.lo[0] || x > T.hi[0])
        return false;
    const int32_t v[3] = {x, 8 * bc[1] + (int32_t)(row & 7u), 8 * bc[2] + (int32_t)(row >> 3)};
    return vox_sat(S, v, v);
}

// the 64 voxel bits of row `row` of block bc ORed into the output: one atomic per word that has a bit (a bit is a voxel
// below dims[0], so its word is one of the row's)
__host__ __device__ inline void vox_row_store(const VoxArgs& A, const int32_t bc[3], uint32_t row, uint64_t mask)
{
    const uint64_t r = (uint64_t)(8 * bc[1] + (int32_t)(row & 7u)) + (uint64_t)A.d[1] * (uint64_t)(8 * bc[2] + (int32_t)(row >> 3));
    const uint64_t w = r * A.wpr + 2u * (uint32_t)bc[0];
    if ((uint32_t)mask) {
        VXRT_VOX_CHECK(kVoxBits, w);
        atom_or(A.bits + w, (uint32_t)mask);
    }
    if ((uint32_t)(mask >> 32)) {
        VXRT_VOX_CHECK(kVoxBits, w + 1u);
        atom_or(A.bits + w + 1u, (uint32_t)(mask >> 32));
    }
}

// Surface item q of a triangle, run by one wave.  `wave.ballot(f)` is the 64-bit mask of f(lane) over the wave's lanes;
// `wave.first()` is true in one lane.
template <class Wave>
__host__ __device__ inline void vox_surface_item(const VoxArgs& A, const VoxTri& T, const VoxSat& S, uint32_t q, const Wave& wave)
{
    VXRT_VOX_COUNT(0);
    uint64_t blocks = wave.ballot([&](uint32_t lane) { return vox_block_hit(A, T, S, q, lane); });
    while (blocks) {
        const uint32_t b = (uint32_t)__builtin_ctzll(blocks);
        blocks &= blocks - 1u;
        int32_t bc[3];
        vox_block_coords(T, 64u * q + b, bc);
        VXRT_VOX_COUNT(1);
        uint64_t rows = wave.ballot([&](uint32_t lane) { return vox_row_hit(A, T, S, bc, lane); });
        while (rows) {
            const uint32_t row = (uint32_t)__builtin_ctzll(rows);
            rows &= rows - 1u;
            VXRT_VOX_COUNT(2);
            const uint64_t mask = wave.ballot([&](uint32_t lane) { return vox_voxel_hit(T, S, bc, row, lane); });
            if (mask && wave.first())
                vox_row_store(A, bc, row, mask);
        }
    }
}

// ---- solid: the toggle of one (triangle, column) ----------------------------------------------------------------------------

// Per-triangle constants, the triangle oriented so that n.x > 0 (v1 and v2 swapped when it was negative).  Edge e runs from
// p[e] to p[e + 1]; (ey, ez) is its inward normal in the yz projection.
struct VoxSolid {
    int32_t py[3], pz[3], ey[3], ez[3];
    bool tie[3];       // the top-left rule: an edge function of exactly 0 counts as inside
    int64_t nx, ny, nz;  // nx > 0
    int64_t q0;          // nx * (v0.x - 128): at most 2^39 * 2^19
    int32_t v0y, v0z;
};

__host__ __device__ inline void vox_solid_setup(const VoxTri& T, VoxSolid& S)
{
    const bool flip = T.n[0] < 0;
    const int order[3] = {0, flip ? 2 : 1, flip ? 1 : 2};
    for (int e = 0; e < 3; ++e) {
        S.py[e] = T.v[order[e]][1];
        S.pz[e] = T.v[order[e]][2];
    }
    for (int e = 0; e < 3; ++e) {
        const int f = e == 2 ? 0 : e + 1;
        S.ey[e] = -(S.pz[f] - S.pz[e]);
        S.ez[e] = S.py[f] - S.py[e];
        S.tie[e] = S.ey[e] > 0 || (S.ey[e] == 0 && S.ez[e] > 0);
    }
    S.nx = flip ? -T.n[0] : T.n[0];
    S.ny = flip ? -T.n[1] : T.n[1];
    S.nz = flip ? -T.n[2] : T.n[2];
    S.q0 = S.nx * (T.v[0][0] - 128);
    S.v0y = T.v[0][1];
    S.v0z = T.v[0][2];
}

// lane = column 64 q + lane of the triangle's centre box (j fastest): when the triangle covers the centre (cy, cz), the
// voxels 0 .. m - 1 of row (j, k) have their centre strictly before the plane; bit m - 1 of the row is toggled.
//   n . (c - v0) < 0  <=>  256 nx i < nx v0.x - ny (cy - v0.y) - nz (cz - v0.z) - 128 nx = a, so m = ceil(a / (256 nx)) cut
//   to 0 .. dims[0]; |a| < 2^58 + 2^59 + 2^59.
__host__ __device__ inline void vox_solid_lane(const VoxArgs& A, const VoxTri& T, const VoxSolid& S, uint32_t q, uint32_t lane)
{
    const uint32_t ny = (uint32_t)(T.chi[0] - T.clo[0] + 1), nz = (uint32_t)(T.chi[1] - T.clo[1] + 1), c = 64u * q + lane;
    if (c >= ny * nz)
        return;
    const int32_t j = T.clo[0] + (int32_t)(c % ny), k = T.clo[1] + (int32_t)(c / ny);
    const int32_t cy = kVoxUnit * j + 128, cz = kVoxUnit * k + 128;
    for (int e = 0; e < 3; ++e) {
        const int64_t E = (int64_t)S.ey[e] * (cy - S.py[e]) + (int64_t)S.ez[e] * (cz - S.pz[e]);
        if (E < 0 || (E == 0 && !S.tie[e]))
            return;
    }
    const int64_t a = S.q0 - S.ny * (cy - S.v0y) - S.nz * (cz - S.v0z);
    const int64_t den = kVoxUnit * S.nx;  // at most 2^47
    if (a <= 0)
        return;  // m = 0
    const uint32_t m = a > den * A.d[0] ? (uint32_t)A.d[0] : (uint32_t)((uint64_t)(a - 1) / (uint64_t)den) + 1u;
    const uint64_t w = ((uint64_t)j + (uint64_t)A.d[1] * (uint64_t)k) * A.wpr + ((m - 1u) >> 5);
    VXRT_VOX_CHECK(kVoxToggle, w);
    vox_atom_xor(A.toggle + w, 1u << ((m - 1u) & 31u));
}

// ---- the last pass: lane = one word of the output ----------------------------------------------------------------------------

// the parity of toggle word g (the kernel ballots it over the words of a row)
__host__ __device__ inline bool vox_final_parity(const VoxArgs& A, uint64_t g)
{
    if (!(A.modes & kVoxSolid))
        return false;
    VXRT_VOX_CHECK(kVoxToggle, g);
    return (__builtin_popcount(A.toggle[g]) & 1) != 0;
}

struct VoxTally {
    uint32_t set, surface, solid;
};

// word g of the output: `higher` is the parity of the toggles in the higher words of its row.  Bit i of the solid word is
// the XOR of the toggles at or above i: a shift-XOR ladder within the word, inverted when `higher` is odd.  The padding bits
// stay 0: no toggle lies at or above dims[0], and the last word of a row has no higher word, so it is never inverted.
__host__ __device__ inline void vox_final_word(const VoxArgs& A, uint64_t g, bool higher, VoxTally& t)
{
    uint32_t solid = 0u;
    if (A.modes & kVoxSolid) {
        VXRT_VOX_CHECK(kVoxToggle, g);
        uint32_t x = A.toggle[g];
        x ^= x >> 1;
        x ^= x >> 2;
        x ^= x >> 4;
        x ^= x >> 8;
        x ^= x >> 16;
        if (higher)
            x = ~x;
        solid = x;
    }
    VXRT_VOX_CHECK(kVoxBits, g);
    const uint32_t surface = A.bits[g];
    const uint32_t out = surface | solid;
    if (solid)
        A.bits[g] = out;
    t.set += (uint32_t)__builtin_popcount(out);
    t.surface += (uint32_t)__builtin_popcount(surface);
    t.solid += (uint32_t)__builtin_popcount(solid);
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_voxelize.hip on a box of d voxels
hipError_t voxelize_mesh(const int32_t* verts, uint32_t nv, const uint32_t* tris, uint32_t nt, const int32_t d[3], uint32_t modes,
                         void* work, uint32_t* bits, vxrt_voxelize_summary* summary, uint32_t work_waves, hipStream_t stream);
#endif

}  // namespace vxrt
