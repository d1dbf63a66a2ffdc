// vxrt_nav.hpp -- navigation fields (include/vxrt.h, vxrt_nav_field / vxrt_nav_paths): the pieces shared by the kernels of
// vxrt_nav.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/nav_check.cpp, through
// tests/tools/hoststub): the workspace layout, the three erosion passes that make the free and walkable bits, the goal
// step, the tile marking, one BFS level of one region word, the next code of one cell and the walk of one path.
//
// Halo.  free() and supported() of the cells of B read the box [origin - (0,1,0), origin + dims + (W-1, H-1, W-1)) of the
// world (W = width, H = height): halo cell (hx, hy, hz) is world cell origin + (hx, hy - 1, hz), so cell (x, y, z) of B is
// halo cell (x, y + 1, z).  Its bits come from k_read_region.
// Bit planes.  Every plane over B is in region bit layout: word xw of row (y, z) holds the cells 32 xw .. 32 xw + 31.
// BFS.  Reverse and level-synchronous, pull-style: at level L a word of an active tile gathers, for every move, the
// frontier bits of the move's targets (funnel-shifted by the move's dx) under the move's sweep mask, and keeps the bits that
// are walkable and not yet visited.  Sweep masks are running ANDs of free rows: above c for a climb, above t for a drop
// (a drop of j shares the first j - 1 rows with the drop of j - 1).  A word writes only itself, so no atomics touch the
// planes.  The frontier of level L lives in plane L & 1; a tile's words there are valid only when the tile's stamp for that
// plane equals L (a tile the level before did not visit holds stale bits, which read as 0).
// Tiles.  32 x 16 x 16 cells: one region word per lane of a 256-lane workgroup.  A tile that found new cells at level L
// marks the tiles that can hold their predecessors (x +-1 word when bit 0 / 31 is set, y - climb .. y + drop, z +-1) for
// level L + 1: an atomicMax of the level into the tile's mark appends the tile to the next list once.  Lists rotate over
// three slots (level L reads L % 3, appends to (L + 1) % 3, clears (L + 2) % 3), so no level sweeps all of B.
// The atomics are vxrt_region.hpp's (plain read-modify-writes on the host).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into an array of the workspace or the outputs against that
// array's size (array: one of the kNav* ids below).  The kernels leave it empty.
#ifndef VXRT_NAV_CHECK
#define VXRT_NAV_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint64_t kNavMaxCells = 1ull << 28;
constexpr uint32_t kNavMaxGoals = 4096, kNavMaxDist = 1u << 24, kNavMaxSteps = 65535;
constexpr uint32_t kNavUnreached = 0xFFFFFFFFu;
constexpr uint8_t kNavNone = 0xFF;
constexpr int kNavTileY = 16, kNavTileZ = 16;  // a tile is 32 x 16 x 16 cells: 256 region words
constexpr uint32_t kNavSlots = 3;              // tile lists in rotation
constexpr uint32_t kNavCtrlWords = 64;  // (a whole section: 256 bytes)
enum { kNavHalo, kNavEx, kNavDx, kNavFy, kNavFree, kNavWalk, kNavVis, kNavFront, kNavDist, kNavStamp, kNavMark, kNavList,
       kNavCtrl, kNavNext, kNavGoals, kNavCells, kNavLengths };
// summary words (vxrt_nav_summary)
enum { kNavSumNodes, kNavSumGoalsUsed, kNavSumGoalsIgnored, kNavSumReached, kNavSumMaxDist, kNavSumLevels, kNavSumTiles,
       kNavSumVisits };

inline bool nav_agent_ok(int32_t w, int32_t h, int32_t climb, int32_t drop)
{
    return w >= 1 && w <= 8 && h >= 1 && h <= 32 && climb >= 0 && climb <= 8 && drop >= 0 && drop <= 32;
}

// the workspace: sections of 32-bit words, each on a 256-byte boundary (include/vxrt.h states the same formula)
struct NavLayout {
    uint64_t halo, ex, dx, fy, free, vis, front[2], dist, stamp, mark, list, ctrl;  // word offsets
    uint64_t total_bytes;
    uint32_t wb, wh;        // words per row of B, of the halo
    uint32_t hy, hz;        // halo rows: dims[1] + H, dims[2] + W - 1
    uint32_t nvox;          // cells of B
    uint64_t nb;            // words of a plane over B
    uint32_t nty, ntz, ntiles;
};

inline bool nav_layout(const int32_t d[3], int32_t w, int32_t h, int32_t climb, int32_t drop, NavLayout& L)
{
    L.nvox = (uint32_t)box_voxels(d, kNavMaxCells);
    if (L.nvox == 0 || !nav_agent_ok(w, h, climb, drop))
        return false;
    L.wb = (uint32_t)region_words_per_row(d[0]);
    L.wh = (uint32_t)(((uint64_t)d[0] + (uint64_t)w - 1u + 31u) >> 5);
    L.hy = (uint32_t)d[1] + (uint32_t)h;
    L.hz = (uint32_t)d[2] + (uint32_t)w - 1u;
    L.nb = (uint64_t)L.wb * (uint64_t)d[1] * (uint64_t)d[2];
    L.nty = ((uint32_t)d[1] + kNavTileY - 1) / kNavTileY;
    L.ntz = ((uint32_t)d[2] + kNavTileZ - 1) / kNavTileZ;
    L.ntiles = L.wb * L.nty * L.ntz;  // <= 2^23
    Sections S;
    L.halo = S.take((uint64_t)L.wh * L.hy * L.hz, 4);
    L.ex = S.take((uint64_t)L.wb * L.hy * L.hz, 4);
    L.dx = S.take((uint64_t)L.wb * (uint64_t)d[1] * L.hz, 4);
    L.fy = S.take((uint64_t)L.wb * (uint64_t)d[1] * L.hz, 4);
    L.free = S.take(L.nb, 4);
    L.vis = S.take(L.nb, 4);
    L.front[0] = S.take(L.nb, 4);
    L.front[1] = S.take(L.nb, 4);
    L.dist = S.take(L.nvox, 4);
    L.stamp = S.take(6u * (uint64_t)L.ntiles, 4);  // stamp, mark and list packed into one section
    L.mark = L.stamp + 2u * (uint64_t)L.ntiles;
    L.list = L.mark + L.ntiles;
    L.ctrl = S.take(kNavCtrlWords, 4);
    L.total_bytes = 4u * S.at;
    return true;
}

// what the nav kernels read and write (device pointers; host pointers in the harness)
struct NavArgs {
    const uint32_t* halo;  // the halo's region words (k_read_region)
    uint32_t* ex;          // halo rows eroded along x: all W empty (wb words per row, hy * hz rows)
    uint32_t* dx;          // halo rows y < dims[1] dilated along x: some of W solid (dims[1] * hz rows)
    uint32_t* fy;          // ex eroded along y over H rows (dims[1] * hz rows)
    uint32_t* free;        // free(c) over B
    uint32_t* walk;        // output: nodes over B
    uint32_t* vis;         // reached nodes
    uint32_t* front[2];    // frontier planes, valid per tile under the stamps
    uint32_t* dist;        // per cell (the output, or the workspace's)
    uint32_t* stamp;       // 2 x ntiles: the level whose frontier a tile's words in plane k hold
    uint32_t* mark;        // ntiles: 1 + the last level the tile was listed for
    uint32_t* list;        // 3 x ntiles
    uint32_t* ctrl;        // [0, 3): list counts
    uint8_t* next;         // output
    uint32_t* summary;     // output: vxrt_nav_summary
    const int32_t* goals;  // 3 per goal
    uint32_t ngoals;
    int32_t o[3], d[3];
    int32_t w, h, climb, drop;
    uint32_t wb, wh, hy, hz, nvox, nty, ntz, ntiles;
    uint64_t nb;
};

// dist: the caller's per-cell output, or NULL for the workspace's
inline void nav_args(NavArgs& A, const NavLayout& L, const int32_t o[3], const int32_t d[3], int32_t w, int32_t h, int32_t climb,
                     int32_t drop, const int32_t* goals, uint32_t ngoals, void* work, uint32_t* walkable, uint8_t* next, uint32_t* dist,
                     uint32_t* summary)
{
    uint32_t* ws = (uint32_t*)work;
    A.halo = ws + L.halo;
    A.ex = ws + L.ex;
    A.dx = ws + L.dx;
    A.fy = ws + L.fy;
    A.free = ws + L.free;
    A.walk = walkable;
    A.vis = ws + L.vis;
    A.front[0] = ws + L.front[0];
    A.front[1] = ws + L.front[1];
    A.dist = dist ? dist : ws + L.dist;
    A.stamp = ws + L.stamp;
    A.mark = ws + L.mark;
    A.list = ws + L.list;
    A.ctrl = ws + L.ctrl;
    A.next = next;
    A.summary = summary;
    A.goals = goals;
    A.ngoals = ngoals;
    for (int k = 0; k < 3; ++k) {
        A.o[k] = o[k];
        A.d[k] = d[k];
    }
    A.w = w;
    A.h = h;
    A.climb = climb;
    A.drop = drop;
    A.wb = L.wb;
    A.wh = L.wh;
    A.hy = L.hy;
    A.hz = L.hz;
    A.nvox = L.nvox;
    A.nty = L.nty;
    A.ntz = L.ntz;
    A.ntiles = L.ntiles;
    A.nb = L.nb;
}

__host__ __device__ inline uint64_t nav_word(const NavArgs& A, uint32_t xw, uint32_t y, uint32_t z)
{
    return (uint64_t)xw + (uint64_t)A.wb * ((uint64_t)y + (uint64_t)A.d[1] * z);
}
__host__ __device__ inline uint32_t nav_cell(const NavArgs& A, uint32_t x, uint32_t y, uint32_t z)
{
    return x + (uint32_t)A.d[0] * (y + (uint32_t)A.d[1] * z);
}
__host__ __device__ inline uint32_t nav_tile(const NavArgs& A, uint32_t xw, uint32_t y, uint32_t z)
{
    return xw + A.wb * (y / kNavTileY + A.nty * (z / kNavTileZ));
}
// the valid bits of word xw of a row of B
__host__ __device__ inline uint32_t nav_row_mask(const NavArgs& A, uint32_t xw)
{
    const uint32_t r = (uint32_t)A.d[0] & 31u;
    return (xw == A.wb - 1u && r) ? (1u << r) - 1u : 0xFFFFFFFFu;
}

// ---- free and walkable bits: three separable passes --------------------------------------------------------------------

// x: word xw of halo row (hy, hz): ex = all of the W voxels x .. x + W - 1 empty; dx (rows hy < dims[1]) = some solid
__host__ __device__ inline void nav_xpass_word(const NavArgs& A, uint32_t xw, uint32_t hy, uint32_t hz)
{
    const uint64_t r = (uint64_t)A.wh * ((uint64_t)hy + (uint64_t)A.hy * hz);
    uint32_t e = 0xFFFFFFFFu, s = 0u;
    for (int i = 0; i < A.w; ++i) {
        const int64_t sx = 32 * (int64_t)xw + i;
        VXRT_NAV_CHECK(kNavHalo, r + (uint64_t)(sx >> 5));
        if (((sx >> 5) + 1) < (int64_t)A.wh)
            VXRT_NAV_CHECK(kNavHalo, r + (uint64_t)(sx >> 5) + 1u);
        const uint32_t g = row_gather32(A.halo + r, A.wh, sx);
        e &= ~g;
        s |= g;
    }
    const uint64_t o = (uint64_t)xw + (uint64_t)A.wb * ((uint64_t)hy + (uint64_t)A.hy * hz);
    VXRT_NAV_CHECK(kNavEx, o);
    A.ex[o] = e;
    if (hy < (uint32_t)A.d[1]) {
        const uint64_t od = (uint64_t)xw + (uint64_t)A.wb * ((uint64_t)hy + (uint64_t)A.d[1] * hz);
        VXRT_NAV_CHECK(kNavDx, od);
        A.dx[od] = s;
    }
}

// y: word xw of row (y, hz), y < dims[1]: the agent's H rows y + 1 .. y + H of the halo (cells y .. y + H - 1) all empty
__host__ __device__ inline void nav_ypass_word(const NavArgs& A, uint32_t xw, uint32_t y, uint32_t hz)
{
    uint32_t f = 0xFFFFFFFFu;
    for (int j = 0; j < A.h; ++j) {
        const uint64_t i = (uint64_t)xw + (uint64_t)A.wb * ((uint64_t)y + 1u + (uint64_t)j + (uint64_t)A.hy * hz);
        VXRT_NAV_CHECK(kNavEx, i);
        f &= A.ex[i];
    }
    const uint64_t o = (uint64_t)xw + (uint64_t)A.wb * ((uint64_t)y + (uint64_t)A.d[1] * hz);
    VXRT_NAV_CHECK(kNavFy, o);
    A.fy[o] = f;
}

// z: word xw of row (y, z) of B: free = the W rows z .. z + W - 1 of fy; walkable = free and some solid voxel in the
// footprint's row below.  Returns the word's nodes.
__host__ __device__ inline uint32_t nav_zpass_word(const NavArgs& A, uint32_t xw, uint32_t y, uint32_t z)
{
    uint32_t f = nav_row_mask(A, xw), s = 0u;
    for (int k = 0; k < A.w; ++k) {
        const uint64_t i = (uint64_t)xw + (uint64_t)A.wb * ((uint64_t)y + (uint64_t)A.d[1] * ((uint64_t)z + (uint64_t)k));
        VXRT_NAV_CHECK(kNavFy, i);
        VXRT_NAV_CHECK(kNavDx, i);
        f &= A.fy[i];
        s |= A.dx[i];
    }
    const uint64_t o = nav_word(A, xw, y, z);
    VXRT_NAV_CHECK(kNavFree, o);
    VXRT_NAV_CHECK(kNavWalk, o);
    A.free[o] = f;
    A.walk[o] = f & s;
    return (uint32_t)__builtin_popcount(f & s);
}

// ---- tile lists ---------------------------------------------------------------------------------------------------------

// list tile t for level lv (once per level)
__host__ __device__ inline void nav_mark_tile(const NavArgs& A, uint32_t lv, uint32_t t)
{
    VXRT_NAV_CHECK(kNavMark, t);
    if (atom_max(A.mark + t, lv + 1u) < lv + 1u) {
        VXRT_NAV_CHECK(kNavCtrl, lv % kNavSlots);
        const uint32_t k = atom_add(A.ctrl + lv % kNavSlots, 1u);
        VXRT_NAV_CHECK(kNavList, (uint64_t)(lv % kNavSlots) * A.ntiles + k);
        A.list[(uint64_t)(lv % kNavSlots) * A.ntiles + k] = t;
    }
}

// list for level lv every tile that can hold a predecessor of a new cell of tile word column tx with cells in rows
// ylo .. yhi, z zlo .. zhi (bit 0 set somewhere: e0; bit 31: e31)
__host__ __device__ inline void nav_mark_around(const NavArgs& A, uint32_t lv, uint32_t tx, bool e0, bool e31, int32_t ylo,
                                                int32_t yhi, int32_t zlo, int32_t zhi)
{
    const int32_t xa = e0 && tx > 0 ? (int32_t)tx - 1 : (int32_t)tx;
    const int32_t xb = e31 && tx + 1u < A.wb ? (int32_t)tx + 1 : (int32_t)tx;
    const int32_t ya = (ylo - A.climb > 0 ? ylo - A.climb : 0) / kNavTileY;
    const int32_t yb = (yhi + A.drop < A.d[1] - 1 ? yhi + A.drop : A.d[1] - 1) / kNavTileY;
    const int32_t za = (zlo > 0 ? zlo - 1 : 0) / kNavTileZ;
    const int32_t zb = (zhi < A.d[2] - 1 ? zhi + 1 : A.d[2] - 1) / kNavTileZ;
    for (int32_t tz = za; tz <= zb; ++tz)
        for (int32_t ty = ya; ty <= yb; ++ty)
            for (int32_t x = xa; x <= xb; ++x)
                nav_mark_tile(A, lv, (uint32_t)x + A.wb * ((uint32_t)ty + A.nty * (uint32_t)tz));
}

// ---- goals ------------------------------------------------------------------------------------------------------------

// goal g: a node of B joins level 0 (frontier plane 0, visited, dist 0) and lists its neighbourhood for level 0.  Returns
// 0 (ignored), 1 (used, already a goal) or 2 (used, a new goal node).
__host__ __device__ inline int nav_goal(const NavArgs& A, uint32_t g)
{
    VXRT_NAV_CHECK(kNavGoals, 3u * g + 2u);
    const int64_t x = (int64_t)A.goals[3u * g] - A.o[0], y = (int64_t)A.goals[3u * g + 1u] - A.o[1],
                  z = (int64_t)A.goals[3u * g + 2u] - A.o[2];
    if (x < 0 || y < 0 || z < 0 || x >= A.d[0] || y >= A.d[1] || z >= A.d[2])
        return 0;
    const uint32_t xw = (uint32_t)x >> 5, bit = 1u << ((uint32_t)x & 31u);
    const uint64_t w = nav_word(A, xw, (uint32_t)y, (uint32_t)z);
    VXRT_NAV_CHECK(kNavWalk, w);
    if (!(A.walk[w] & bit))
        return 0;
    VXRT_NAV_CHECK(kNavFront, w);
    VXRT_NAV_CHECK(kNavVis, w);
    atom_or(A.front[0] + w, bit);
    const bool fresh = !(atom_or(A.vis + w, bit) & bit);
    const uint32_t t = nav_tile(A, xw, (uint32_t)y, (uint32_t)z);
    VXRT_NAV_CHECK(kNavStamp, t);
    A.stamp[t] = 0u;
    const uint32_t c = nav_cell(A, (uint32_t)x, (uint32_t)y, (uint32_t)z);
    VXRT_NAV_CHECK(kNavDist, c);
    A.dist[c] = 0u;
    nav_mark_around(A, 0u, xw, bit == 1u, bit == 0x80000000u, (int32_t)y, (int32_t)y, (int32_t)z, (int32_t)z);
    return fresh ? 2 : 1;
}

// ---- one BFS level ----------------------------------------------------------------------------------------------------

// word xw of frontier plane lv & 1 at (y, z) in B, 0 outside B or in a tile whose stamp is not lv
__host__ __device__ inline uint32_t nav_front(const NavArgs& A, uint32_t lv, int64_t xw, int64_t y, int64_t z)
{
    if (xw < 0 || y < 0 || z < 0 || xw >= (int64_t)A.wb || y >= A.d[1] || z >= A.d[2])
        return 0u;
    const uint32_t t = nav_tile(A, (uint32_t)xw, (uint32_t)y, (uint32_t)z);
    VXRT_NAV_CHECK(kNavStamp, (uint64_t)(lv & 1u) * A.ntiles + t);
    if (A.stamp[(uint64_t)(lv & 1u) * A.ntiles + t] != lv)
        return 0u;
    const uint64_t w = nav_word(A, (uint32_t)xw, (uint32_t)y, (uint32_t)z);
    VXRT_NAV_CHECK(kNavFront, w);
    return A.front[lv & 1u][w];
}

__host__ __device__ inline uint32_t nav_free_word(const NavArgs& A, int64_t xw, int64_t y, int64_t z)
{
    if (xw < 0 || y < 0 || z < 0 || xw >= (int64_t)A.wb || y >= A.d[1] || z >= A.d[2])
        return 0u;
    const uint64_t w = nav_word(A, (uint32_t)xw, (uint32_t)y, (uint32_t)z);
    VXRT_NAV_CHECK(kNavFree, w);
    return A.free[w];
}

// bit b of the result = bit b + dx of the row (y, z) of a plane around word xw, dx in {-1, 0, 1}
template <typename Get>
__host__ __device__ inline uint32_t nav_shifted(Get get, int64_t xw, int dx)
{
    const uint32_t m = get(xw);
    if (dx == 0)
        return m;
    if (dx > 0)
        return (m >> 1) | (get(xw + 1) << 31);
    return (m << 1) | (get(xw - 1) >> 31);
}

// the direction of index k (+x, -x, +z, -z)
__host__ __device__ inline void nav_dir(int k, int& dx, int& dz)
{
    dx = k == 0 ? 1 : (k == 1 ? -1 : 0);
    dz = k == 2 ? 1 : (k == 3 ? -1 : 0);
}

// level lv -> lv + 1 for word xw of row (y, z) of B: the new cells (walkable, not visited, with a valid move onto a
// frontier cell), written to frontier plane (lv + 1) & 1, visited and dist.  Returns the new bits.
__host__ __device__ inline uint32_t nav_level_word(const NavArgs& A, uint32_t lv, uint32_t xw, uint32_t y, uint32_t z)
{
    const uint64_t w = nav_word(A, xw, y, z);
    VXRT_NAV_CHECK(kNavWalk, w);
    VXRT_NAV_CHECK(kNavVis, w);
    const uint32_t cand = A.walk[w] & ~A.vis[w];
    uint32_t acc = 0u;
    if (cand) {
        for (int k = 0; k < 4; ++k) {
            int dx, dz;
            nav_dir(k, dx, dz);
            const int64_t tz = (int64_t)z + dz;
            if (tz < 0 || tz >= A.d[2])
                continue;
            auto fr = [&](int64_t yy) {
                return nav_shifted([&](int64_t q) { return nav_front(A, lv, q, yy, tz); }, (int64_t)xw, dx);
            };
            acc |= fr((int64_t)y);
            uint32_t a = 0xFFFFFFFFu;  // climb: free above c
            for (int j = 1; j <= A.climb && (int64_t)y + j < A.d[1]; ++j) {
                a &= nav_free_word(A, (int64_t)xw, (int64_t)y + j, (int64_t)z);
                if (!(a & cand))
                    break;
                acc |= a & fr((int64_t)y + j);
            }
            uint32_t g = 0xFFFFFFFFu;  // drop: free above t, up to c's row
            for (int j = 1; j <= A.drop && (int64_t)y - j >= 0; ++j) {
                const int64_t yr = (int64_t)y - j + 1;
                g &= nav_shifted([&](int64_t q) { return nav_free_word(A, q, yr, tz); }, (int64_t)xw, dx);
                if (!(g & cand))
                    break;
                acc |= g & fr((int64_t)y - j);
            }
        }
    }
    const uint32_t nw = cand & acc;
    VXRT_NAV_CHECK(kNavFront, w);
    A.front[(lv + 1u) & 1u][w] = nw;
    if (nw) {
        A.vis[w] |= nw;
        for (uint32_t m = nw; m; m &= m - 1u) {
            const uint32_t c = nav_cell(A, 32u * xw + (uint32_t)__builtin_ctz(m), y, z);
            VXRT_NAV_CHECK(kNavDist, c);
            A.dist[c] = lv + 1u;
        }
    }
    return nw;
}

// ---- next codes and paths ---------------------------------------------------------------------------------------------

__host__ __device__ inline bool nav_free_at(const NavArgs& A, int64_t x, int64_t y, int64_t z)
{
    if (x < 0 || x >= A.d[0])
        return false;
    return (nav_free_word(A, x >> 5, y, z) >> (x & 31)) & 1u;
}

__host__ __device__ inline uint32_t nav_dist_at(const NavArgs& A, int64_t x, int64_t y, int64_t z)
{
    if (x < 0 || y < 0 || z < 0 || x >= A.d[0] || y >= A.d[1] || z >= A.d[2])
        return kNavUnreached;
    const uint32_t c = nav_cell(A, (uint32_t)x, (uint32_t)y, (uint32_t)z);
    VXRT_NAV_CHECK(kNavDist, c);
    return A.dist[c];
}

// the next code of cell (x, y, z) of B
__host__ __device__ inline uint8_t nav_next_cell(const NavArgs& A, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t D = nav_dist_at(A, x, y, z);
    if (D == kNavUnreached)
        return kNavNone;
    if (D == 0u)
        return 0;
    const int per = 1 + A.climb + A.drop;
    for (int k = 0; k < 4; ++k) {
        int dx, dz;
        nav_dir(k, dx, dz);
        const int64_t tx = (int64_t)x + dx, tz = (int64_t)z + dz;
        if (tx < 0 || tx >= A.d[0] || tz < 0 || tz >= A.d[2])
            continue;
        const int base = 1 + k * per;
        if (nav_dist_at(A, tx, y, tz) == D - 1u)
            return (uint8_t)base;
        for (int j = 1; j <= A.climb && (int64_t)y + j < A.d[1]; ++j) {
            if (!nav_free_at(A, x, (int64_t)y + j, z))
                break;
            if (nav_dist_at(A, tx, (int64_t)y + j, tz) == D - 1u)
                return (uint8_t)(base + j);
        }
        for (int j = 1; j <= A.drop && (int64_t)y - j >= 0; ++j) {
            if (!nav_free_at(A, tx, (int64_t)y - j + 1, tz))
                break;
            if (nav_dist_at(A, tx, (int64_t)y - j, tz) == D - 1u)
                return (uint8_t)(base + A.climb + j);
        }
    }
    return kNavNone;  // not reached for a field of this call: a reachable cell has a move one level down
}

// the move of code c (1 .. 4 (1 + climb + drop)); false for any other code
__host__ __device__ inline bool nav_decode(uint32_t c, int32_t climb, int32_t drop, int& dx, int& dy, int& dz)
{
    const uint32_t per = 1u + (uint32_t)climb + (uint32_t)drop;
    if (c < 1u || c > 4u * per)
        return false;
    const uint32_t k = (c - 1u) / per, i = (c - 1u) % per;
    nav_dir((int)k, dx, dz);
    dy = i == 0 ? 0 : (i <= (uint32_t)climb ? (int)i : -(int)(i - (uint32_t)climb));
    return true;
}

struct NavPathArgs {
    const uint8_t* next;
    const int32_t* starts;
    int32_t* cells;  // or NULL
    uint32_t* lengths;
    uint32_t* status;
    uint64_t n;
    uint32_t max_steps;
    int32_t o[3], d[3];
    int32_t climb, drop;
};

// the walk of start i: cells (when kept), length and status
__host__ __device__ inline void nav_path(const NavPathArgs& P, uint64_t i)
{
    VXRT_NAV_CHECK(kNavGoals, 3u * i + 2u);
    int64_t p[3] = {P.starts[3u * i], P.starts[3u * i + 1u], P.starts[3u * i + 2u]};
    int32_t* out = P.cells ? P.cells + 3u * (uint64_t)(P.max_steps + 1u) * i : nullptr;
    auto put = [&](uint32_t s) {
        VXRT_NAV_CHECK(kNavCells, 3u * ((uint64_t)(P.max_steps + 1u) * i + s) + 2u);
        for (int k = 0; k < 3; ++k)
            out[3u * s + (uint32_t)k] = (int32_t)p[k];
    };
    auto inside = [&]() {
        for (int k = 0; k < 3; ++k)
            if (p[k] < P.o[k] || p[k] - P.o[k] >= P.d[k])
                return false;
        return true;
    };
    uint32_t steps = 0, st;
    if (!inside()) {
        st = 3u;  // VXRT_NAV_OUTSIDE
    } else {
        if (out)
            put(0);
        for (;;) {
            const uint64_t c = (uint64_t)(p[0] - P.o[0]) + (uint64_t)P.d[0] * ((uint64_t)(p[1] - P.o[1]) + (uint64_t)P.d[1] * (uint64_t)(p[2] - P.o[2]));
            VXRT_NAV_CHECK(kNavNext, c);
            const uint32_t code = P.next[c];
            if (code == 0u) {
                st = 0u;  // VXRT_NAV_AT_GOAL
                break;
            }
            int dx, dy, dz;
            if (!nav_decode(code, P.climb, P.drop, dx, dy, dz)) {
                st = 1u;  // VXRT_NAV_NO_PATH
                break;
            }
            if (steps == P.max_steps) {
                st = 2u;  // VXRT_NAV_TRUNCATED
                break;
            }
            p[0] += dx;
            p[1] += dy;
            p[2] += dz;
            if (!inside()) {  // a code no field writes: stop on the last cell inside
                p[0] -= dx;
                p[1] -= dy;
                p[2] -= dz;
                st = 1u;
                break;
            }
            ++steps;
            if (out)
                put(steps);
        }
    }
    if (out)
        for (uint32_t s = st == 3u ? 0u : steps + 1u; s <= P.max_steps; ++s)
            put(s);
    VXRT_NAV_CHECK(kNavLengths, i);
    P.lengths[i] = steps;
    P.status[i] = st;
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_nav.hip
hipError_t nav_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], const vxrt_nav_agent& ag, const int32_t* goals,
                     uint32_t ngoals, uint32_t max_dist, void* work, uint32_t* walkable, uint8_t* next, uint32_t* dist,
                     vxrt_nav_summary* summary, hipStream_t stream);
hipError_t nav_paths(const NavPathArgs& P, hipStream_t stream);
#endif

}  // namespace vxrt
