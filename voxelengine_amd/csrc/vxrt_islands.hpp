// vxrt_islands.hpp -- floating-island detection (include/vxrt.h, vxrt_find_islands): the pieces shared by the kernels of
// vxrt_islands.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/islands_check.cpp, through
// tests/tools/hoststub): the workspace layout, run starts, the union-find over uint32 parents, the tile-local union, the
// border merge, the flatten step with its anchor test, the island rank and the table row.
//
// Union-find.  parent[i] <= i always: a link hangs the larger root under the smaller one with atomicMin, and the path
// halving of a find lowers a parent to its grandparent with atomicMin too.  Every tree's root is therefore the minimum index
// of its component, whatever order the races resolve in, and the flattened parent is the component id minus 1.  A union
// whose atomicMin finds the larger root already linked elsewhere goes on with that parent, so no link is lost.
// The atomics are vxrt_region.hpp's (plain read-modify-writes on the host).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into an array of the workspace, the LDS tile or the
// outputs against that array's size (array: one of the kIsl* ids below).  The kernels leave it empty.
#ifndef VXRT_ISL_CHECK
#define VXRT_ISL_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint64_t kIslMaxVoxels = 1ull << 28;
constexpr uint32_t kIslEmpty = 0xFFFFFFFFu;  // parent of an empty voxel
constexpr int kIslTileY = 16, kIslTileZ = 16;  // a tile is 32 x 16 x 16 voxels: one region word per row, 256 rows
constexpr uint32_t kIslTileRows = kIslTileY * kIslTileZ;
constexpr uint32_t kIslTileVoxels = 32u * kIslTileRows;  // 8192: 32 KiB of LDS parents
constexpr uint32_t kIslScanBlock = 1024;                 // words per block of the island scan
constexpr uint32_t kIslAnchorMask = 0x7Fu;               // six faces and the floor
enum { kIslBits, kIslParent, kIslRoots, kIslAnchor, kIslPrefix, kIslBlocks, kIslFloating, kIslLabels, kIslTable, kIslTile };

// the workspace: sections of 32-bit words, each on a 256-byte boundary
struct IslandsLayout {
    uint64_t bits, parent, roots, anchor, prefix, blocks;  // word offsets
    uint64_t total_bytes;
    uint32_t wpr;     // words per region row
    uint32_t nvox;    // dims[0] * dims[1] * dims[2] <= 2^28
    uint32_t nwords;  // words of each one-bit-per-voxel section: ceil(nvox / 64) * 2 (a wave writes two)
    uint32_t nblocks; // scan blocks of kIslScanBlock words
    uint64_t nbits;   // words of the region bits: wpr * dims[1] * dims[2]
};

inline bool islands_layout(const int32_t d[3], IslandsLayout& L)
{
    L.nvox = (uint32_t)box_voxels(d, kIslMaxVoxels);
    if (L.nvox == 0)
        return false;
    L.wpr = (uint32_t)region_words_per_row(d[0]);
    L.nbits = region_words(d);
    L.nwords = (uint32_t)((((uint64_t)L.nvox + 63u) >> 6) << 1);
    L.nblocks = (L.nwords + kIslScanBlock - 1) / kIslScanBlock;
    Sections S;
    L.bits = S.take(L.nbits, 4);
    L.parent = S.take(L.nvox, 4);
    L.roots = S.take(L.nwords, 4);
    L.anchor = S.take(L.nwords, 4);
    L.prefix = S.take(L.nwords, 4);
    L.blocks = S.take(L.nblocks, 4);
    L.total_bytes = 4u * S.at;
    return true;
}

// what the island kernels read and write (device pointers; host pointers in the harness)
struct IslandsArgs {
    const uint32_t* bits;  // the box's region words (k_read_region)
    uint32_t* parent;      // one per voxel, region order
    uint32_t* roots;       // one bit per voxel index: a root; later, a root of an island
    uint32_t* anchor;      // one bit per voxel index: a root whose component holds an anchor voxel
    uint32_t* prefix;      // per roots word: island roots before it in its scan block
    uint32_t* blocks;      // per scan block: island roots before the block
    uint32_t* floating;    // output: region words
    uint32_t* labels;      // output or NULL
    int32_t* table;        // output or NULL: 8 words per row (vxrt_island)
    uint32_t* summary;     // output: components, islands, island_voxels
    uint32_t max_islands;
    uint32_t anchors;
    int32_t d[3], o[3];
    uint32_t wpr, nvox, nwords, nblocks;
    uint64_t nbits;
};

inline void islands_args(IslandsArgs& A, const IslandsLayout& L, const int32_t o[3], const int32_t d[3], uint32_t anchors, void* work,
                         uint32_t* floating, uint32_t* labels, int32_t* table, uint32_t max_islands, uint32_t* summary)
{
    uint32_t* ws = (uint32_t*)work;
    A.bits = ws + L.bits;
    A.parent = ws + L.parent;
    A.roots = ws + L.roots;
    A.anchor = ws + L.anchor;
    A.prefix = ws + L.prefix;
    A.blocks = ws + L.blocks;
    A.floating = floating;
    A.labels = labels;
    A.table = max_islands ? table : nullptr;
    A.summary = summary;
    A.max_islands = max_islands;
    A.anchors = anchors;
    for (int k = 0; k < 3; ++k) {
        A.d[k] = d[k];
        A.o[k] = o[k];
    }
    A.wpr = L.wpr;
    A.nvox = L.nvox;
    A.nwords = L.nwords;
    A.nblocks = L.nblocks;
    A.nbits = L.nbits;
}

// the first bit of the run of set bits of w that holds bit b (bit b set): one past the highest clear bit below b
__host__ __device__ inline int isl_run_start(uint32_t w, int b)
{
    const uint32_t below = ~w & ((1u << b) - 1u);  // b = 0: no bit below
    return below ? 32 - __builtin_clz(below) : 0;
}

// the bits where a run of the pairs (a & b) begins: one union per run, the run itself links the rest
__host__ __device__ inline uint32_t isl_pair_starts(uint32_t a, uint32_t b)
{
    const uint32_t ov = a & b;
    return ov & ~(ov << 1);
}

// root of x with path halving; array is kIslParent (global) or kIslTile (LDS)
template <int kArray>
__host__ __device__ inline uint32_t isl_find(uint32_t* P, uint32_t x)
{
    for (;;) {
        VXRT_ISL_CHECK(kArray, x);
        const uint32_t p = atom_load(P + x);
        if (p == x)
            return x;
        VXRT_ISL_CHECK(kArray, p);
        const uint32_t g = atom_load(P + p);
        if (g == p)
            return p;
        atom_min(P + x, g);
        x = g;
    }
}

// unite the trees of a and b: the larger root is hung under the smaller
template <int kArray>
__host__ __device__ inline void isl_union(uint32_t* P, uint32_t a, uint32_t b)
{
    for (;;) {
        a = isl_find<kArray>(P, a);
        b = isl_find<kArray>(P, b);
        if (a == b)
            return;
        if (a > b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        VXRT_ISL_CHECK(kArray, b);
        const uint32_t old = atom_min(P + b, a);
        if (old == b)
            return;
        b = old;  // b had been linked meanwhile: unite a with what it now hangs under
    }
}

__host__ __device__ inline uint32_t isl_index(const IslandsArgs& A, uint32_t x, uint32_t y, uint32_t z)
{
    return x + (uint32_t)A.d[0] * (y + (uint32_t)A.d[1] * z);
}

// ---- tile-local union: tile (tx, ty, tz) covers region word tx of rows y in [16 ty, 16 ty + 16), z likewise; row
// r = ly + 16 lz of the tile is lane r of the workgroup, and tile voxel (x, r) has the local index x + 32 r.  Local order is
// the region order restricted to the tile, so a local minimum is the global minimum of the tile's piece.

// the region word of tile row r (0 outside the box)
__host__ __device__ inline uint32_t isl_tile_row(const IslandsArgs& A, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t r)
{
    const uint32_t y = ty * kIslTileY + (r & (kIslTileY - 1)), z = tz * kIslTileZ + r / kIslTileY;
    if (y >= (uint32_t)A.d[1] || z >= (uint32_t)A.d[2])
        return 0u;
    const uint64_t w = (uint64_t)tx + (uint64_t)A.wpr * ((uint64_t)y + (uint64_t)A.d[1] * z);
    VXRT_ISL_CHECK(kIslBits, w);
    return A.bits[w];
}

// the initial local parent of tile voxel (x, r) whose row word is w: the start of its run along x (an empty voxel: itself)
__host__ __device__ inline void isl_tile_init_voxel(uint32_t* lp, uint32_t w, uint32_t x, uint32_t r)
{
    VXRT_ISL_CHECK(kIslTile, 32u * r + x);
    lp[32u * r + x] = 32u * r + (uint32_t)(((w >> x) & 1u) ? isl_run_start(w, (int)x) : (int)x);
}

// the unions of row r with the rows below it in y and z inside the tile, one per run of face pairs
__host__ __device__ inline void isl_tile_union_row(uint32_t* lp, const uint32_t* rows, uint32_t r)
{
    const uint32_t w = rows[r];
    if (!w)
        return;
    for (int k = 0; k < 2; ++k) {
        const uint32_t step = k == 0 ? 1u : (uint32_t)kIslTileY;
        if ((k == 0 ? (r & (kIslTileY - 1)) : r / kIslTileY) == 0)
            continue;
        for (uint32_t s = isl_pair_starts(w, rows[r - step]); s; s &= s - 1u) {
            const uint32_t x = (uint32_t)__builtin_ctz(s);
            isl_union<kIslTile>(lp, 32u * r + x, 32u * (r - step) + x);
        }
    }
}

// the global parent of tile voxel (x, r): the region index of its tile-local root, kIslEmpty for an empty voxel.  Returns
// false (nothing to write) for a voxel outside the box.
__host__ __device__ inline bool isl_tile_parent(const IslandsArgs& A, uint32_t* lp, const uint32_t* rows, uint32_t tx,
                                                uint32_t ty, uint32_t tz, uint32_t x, uint32_t r, uint32_t& g, uint32_t& val)
{
    const uint32_t ly = r & (kIslTileY - 1), lz = r / kIslTileY;
    const uint32_t gx = 32u * tx + x, gy = ty * kIslTileY + ly, gz = tz * kIslTileZ + lz;
    if (gx >= (uint32_t)A.d[0] || gy >= (uint32_t)A.d[1] || gz >= (uint32_t)A.d[2])
        return false;
    g = isl_index(A, gx, gy, gz);
    if (!((rows[r] >> x) & 1u)) {
        val = kIslEmpty;
        return true;
    }
    const uint32_t l = isl_find<kIslTile>(lp, 32u * r + x);
    val = isl_index(A, 32u * tx + (l & 31u), ty * kIslTileY + ((l >> 5) & (kIslTileY - 1)), tz * kIslTileZ + (l >> 5) / kIslTileY);
    return true;
}

// ---- border merge: region word (xw, y, z) against its neighbours across tile borders, in global parents: the last voxel of
// word xw - 1 (every word border is a tile border), the row below in y when y is a tile's first row, likewise in z
__host__ __device__ inline void isl_merge_word(const IslandsArgs& A, uint32_t xw, uint32_t y, uint32_t z)
{
    const uint64_t wi = (uint64_t)xw + (uint64_t)A.wpr * ((uint64_t)y + (uint64_t)A.d[1] * z);
    VXRT_ISL_CHECK(kIslBits, wi);
    const uint32_t w = A.bits[wi];
    if (!w)
        return;
    if (xw > 0 && (w & 1u)) {
        VXRT_ISL_CHECK(kIslBits, wi - 1);
        if (A.bits[wi - 1] >> 31)
            isl_union<kIslParent>(A.parent, isl_index(A, 32u * xw, y, z), isl_index(A, 32u * xw - 1u, y, z));
    }
    for (int k = 0; k < 2; ++k) {
        const uint32_t c = k == 0 ? y : z;
        if (c == 0 || c % (k == 0 ? kIslTileY : kIslTileZ) != 0)
            continue;
        const uint64_t step = k == 0 ? (uint64_t)A.wpr : (uint64_t)A.wpr * (uint64_t)A.d[1];
        VXRT_ISL_CHECK(kIslBits, wi - step);
        for (uint32_t s = isl_pair_starts(w, A.bits[wi - step]); s; s &= s - 1u) {
            const uint32_t x = 32u * xw + (uint32_t)__builtin_ctz(s);
            isl_union<kIslParent>(A.parent, isl_index(A, x, y, z), k == 0 ? isl_index(A, x, y - 1, z) : isl_index(A, x, y, z - 1));
        }
    }
}

// ---- flatten: voxel i of the box gets its root (the component id - 1) as parent and label

// an anchor voxel under A.anchors (x, y, z in the box)
__host__ __device__ inline bool isl_is_anchor(const IslandsArgs& A, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t m = A.anchors;
    const uint32_t c[3] = {x, y, z};
    for (int k = 0; k < 3; ++k) {
        if (((m >> (2 * k)) & 1u) && c[k] == 0)
            return true;
        if (((m >> (2 * k + 1)) & 1u) && c[k] == (uint32_t)A.d[k] - 1u)
            return true;
    }
    return (m & 0x40u) && (int64_t)A.o[1] + y == 0;
}

// voxel i < nvox: false for an empty voxel (label 0); otherwise its root, written as its parent and label, and whether the
// voxel is an anchor voxel
__host__ __device__ inline bool isl_flatten_voxel(const IslandsArgs& A, uint32_t i, uint32_t& root, bool& anchor)
{
    VXRT_ISL_CHECK(kIslParent, i);
    const uint32_t p = A.parent[i];
    if (p == kIslEmpty) {
        if (A.labels) {
            VXRT_ISL_CHECK(kIslLabels, i);
            A.labels[i] = 0u;
        }
        return false;
    }
    root = isl_find<kIslParent>(A.parent, i);
    A.parent[i] = root;
    if (A.labels) {
        VXRT_ISL_CHECK(kIslLabels, i);
        A.labels[i] = root + 1u;
    }
    const uint32_t x = i % (uint32_t)A.d[0], t = i / (uint32_t)A.d[0];
    anchor = isl_is_anchor(A, x, t % (uint32_t)A.d[1], t / (uint32_t)A.d[1]);
    return true;
}

// the anchored bit of a root, set once (a load first: a big component's anchor voxels all name the same root)
__host__ __device__ inline void isl_mark_anchor(const IslandsArgs& A, uint32_t root)
{
    VXRT_ISL_CHECK(kIslAnchor, root >> 5);
    const uint32_t bit = 1u << (root & 31u);
    if (!(atom_load(A.anchor + (root >> 5)) & bit))
        atom_or(A.anchor + (root >> 5), bit);
}

// ---- islands: after the scan, roots word w holds the island roots, prefix[w] the island roots before w in its block and
// blocks[b] those before block b

// island roots of word w: roots that no anchor voxel names
__host__ __device__ inline uint32_t isl_island_word(const IslandsArgs& A, uint32_t w)
{
    VXRT_ISL_CHECK(kIslRoots, w);
    VXRT_ISL_CHECK(kIslAnchor, w);
    return A.roots[w] & ~A.anchor[w];
}

// the row of island root r in the table (its rank among the island roots in ascending index)
__host__ __device__ inline uint32_t isl_rank(const IslandsArgs& A, uint32_t r)
{
    const uint32_t w = r >> 5;
    VXRT_ISL_CHECK(kIslRoots, w);
    VXRT_ISL_CHECK(kIslPrefix, w);
    VXRT_ISL_CHECK(kIslBlocks, w / kIslScanBlock);
    return A.blocks[w / kIslScanBlock] + A.prefix[w] + (uint32_t)__builtin_popcount(A.roots[w] & ((1u << (r & 31u)) - 1u));
}

// the table row of island root r before any voxel is counted
__host__ __device__ inline void isl_init_row(const IslandsArgs& A, uint32_t rank, uint32_t r)
{
    VXRT_ISL_CHECK(kIslTable, rank);
    int32_t* row = A.table + 8u * (uint64_t)rank;
    row[0] = (int32_t)(r + 1u);
    row[1] = 0;
    for (int k = 0; k < 3; ++k) {
        row[2 + k] = 0x7FFFFFFF;
        row[5 + k] = (int32_t)0x80000000;
    }
}

// voxel (x, y, z) of the box, x < dims[0]: whether it belongs to an island, and then the island's table row (or
// 0xFFFFFFFF past max_islands / without a table)
__host__ __device__ inline bool isl_voxel_island(const IslandsArgs& A, uint32_t w, uint32_t x, uint32_t y, uint32_t z,
                                                 uint32_t& rank)
{
    if (!((w >> (x & 31u)) & 1u))
        return false;
    const uint32_t i = isl_index(A, x, y, z);
    VXRT_ISL_CHECK(kIslParent, i);
    const uint32_t r = A.parent[i];
    if (r == kIslEmpty)  // a solid bit always has a root; never index the root bits with the empty mark
        return false;
    VXRT_ISL_CHECK(kIslRoots, r >> 5);
    if (!((A.roots[r >> 5] >> (r & 31u)) & 1u))
        return false;
    rank = 0xFFFFFFFFu;
    if (A.table) {
        const uint32_t k = isl_rank(A, r);
        if (k < A.max_islands)
            rank = k;
    }
    return true;
}

// the voxels and box of a table row grown by n voxels whose world box is lo .. hi (inclusive)
__host__ __device__ inline void isl_add_to_row(const IslandsArgs& A, uint32_t rank, uint32_t n, const int32_t lo[3],
                                               const int32_t hi[3])
{
    VXRT_ISL_CHECK(kIslTable, rank);
    int32_t* row = A.table + 8u * (uint64_t)rank;
    atom_add((uint32_t*)row + 1, n);
    for (int k = 0; k < 3; ++k) {
        atom_min(row + 2 + k, lo[k]);
        atom_max(row + 5 + k, hi[k] + 1);
    }
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_islands.hip on the box o, d
hipError_t find_islands(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t anchors, void* work,
                        uint32_t* floating, uint32_t* labels, vxrt_island* table, uint32_t max_islands,
                        vxrt_island_summary* summary, hipStream_t stream);
#endif

}  // namespace vxrt
