// vxrt_transform.hpp -- voxel stamps rotated and mirrored (include/vxrt.h, vxrt_orientation_* / vxrt_transform_stamp): the
// pieces shared by the kernels of vxrt_transform.hip, the host side in vxrt_api_query.hip and the host harnesses of the tests
// (tests/tools/transform_check.cpp, transform_args_check.cpp, through tests/tools/hoststub): the orientation checks and
// algebra behind the C helpers, the limits and the launch plan, and the per-lane work of both kernels.
//
// An orientation is a signed axis permutation: destination axis k runs along source axis axis[k], against it when bit k of
// `flip` is set.  Source voxel p lands at q with q[k] = flip bit k ? sd[axis[k]] - 1 - p[axis[k]] : p[axis[k]].
//
// COPY class (axis[0] == 0).  Rows move whole.  One lane per destination word, lanes along the words of a row: the word is
// word j of the source row the row index maps to (its last word cut to sd[0] bits), or with an x flip the bit reversal of
// the 32 source bits that start at bit sd[0] - 32 (j + 1) (row_gather32: 0 outside the row).
// TRANSPOSE class (axis[0] = s != 0).  Destination x runs along source axis s, source x becomes a destination row index, the
// third source axis t is plain indexing.  A workgroup takes a tile of kTrTJ destination words (32 * kTrTJ source rows along
// s) by kTrTX source x-words at one t, in three phases around two LDS images:
//   load        lanes along the x-words of a source row (contiguous global loads), rows along s; rows outside [0, sd[s]),
//               words outside the row and the bits beyond sd[0] read 0.  With a flip of destination x, destination word j
//               holds the rows sd[s] - 32 (j + 1) .. sd[s] - 32 j - 1: the tile's rows are index arithmetic, not aligned.
//   transpose   a 32-lane half of a wave holds one x-word of 32 consecutive rows and transposes the 32 x 32 bit matrix in
//               five butterfly rounds (partner lanes 16, 8, 4, 2, 1; tr_combine is one round of one lane); lane i then
//               holds the destination word of source x = x0 + i, bit-reversed where destination x is flipped.
//   store       lanes along the destination words of a destination row (contiguous global stores); rows beyond sd[0] and
//               words beyond the destination row are not stored.
// Both LDS images have their rows padded by one word: the column accesses of the transpose phase (stride = row pitch) then
// hit 32 different banks, where the power-of-two pitch would put all 32 lanes of a half on two.
// Every destination word is written exactly once, by the one lane that owns it; the summary is tallied per lane over the
// words the lane stores (count and inclusive bounds in destination coordinates).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into the source, the destination, the summary or an LDS
// image against that array's size (array: one of the kTr* ids below).  The kernels leave it empty.
#ifndef VXRT_TRANSFORM_CHECK
#define VXRT_TRANSFORM_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint64_t kTransformMaxWords = 1ull << 31;
enum { kTrSrc, kTrDst, kTrSum, kTrLdsIn, kTrLdsOut, kTrArrays };
constexpr uint32_t kTrSumWords = 8;  // vxrt_transform_summary as words: voxels (2), set_min (3), set_max (3)
constexpr uint32_t kTrSumMin = 2, kTrSumMax = 5;

// the tile of the TRANSPOSE class: kTrTJ destination words by kTrTX source x-words, 256 lanes
constexpr uint32_t kTrTJ = 8, kTrTX = 16, kTrLanes = 256;
constexpr uint32_t kTrRows = 32u * kTrTJ;                  // source rows of a tile (along s)
constexpr uint32_t kTrXRows = 32u * kTrTX;                 // destination rows of a tile (along source x)
constexpr uint32_t kTrPitchIn = kTrTX + 1u, kTrPitchOut = kTrTJ + 1u;
constexpr uint32_t kTrLdsInWords = kTrRows * kTrPitchIn, kTrLdsOutWords = kTrXRows * kTrPitchOut;
constexpr uint32_t kTrLoads = kTrRows * kTrTX / kTrLanes;  // words a lane loads, and stores, per tile
constexpr uint32_t kTrBlocks = kTrTJ * kTrTX / (kTrLanes / 32u);  // 32 x 32 blocks a half-wave transposes per tile
static_assert(kTrRows * kTrTX % kTrLanes == 0 && kTrTJ * kTrTX % (kTrLanes / 32u) == 0, "tile shape");
// the workgroups of a launch: the lanes walk the words (COPY) or the tiles (TRANSPOSE) with this stride, so that a call
// ends in a bounded number of summary atomics
constexpr uint32_t kTrMaxGroups = 2048;

// Division by a divisor fixed for the launch, for numerators below 2^31 (every word, row and tile index of a call is): with
// l = ceil(log2 d) and m = ceil(2^(31 + l) / d), which fits 32 bits, n / d = (n * m) >> (31 + l) exactly (Granlund and
// Montgomery 1994, theorem 4.2 with N = 31).  A multiply-high and a shift where the division would take some twenty
// instructions per word.
struct TrDiv {
    uint32_t m, sh;
};

inline TrDiv tr_div_by(uint32_t d)
{
    uint32_t l = 0;
    while ((1ull << l) < d)
        ++l;
    const uint64_t p = 1ull << (31u + l);
    return TrDiv{(uint32_t)((p + d - 1u) / d), 31u + l};
}

__host__ __device__ inline uint32_t tr_div(uint32_t n, const TrDiv& d) { return (uint32_t)(((uint64_t)n * d.m) >> d.sh); }

// ---- host: the orientation algebra behind the C helpers ---------------------------------------------------------------------
struct Orient {
    int32_t axis[3];
    uint32_t flip;
};

inline bool orient_valid(const Orient& o)
{
    uint32_t seen = 0u;
    for (int k = 0; k < 3; ++k) {
        if (o.axis[k] < 0 || o.axis[k] > 2)
            return false;
        seen |= 1u << o.axis[k];
    }
    return seen == 7u && o.flip < 8u;
}

// a first, then b
inline Orient orient_compose(const Orient& a, const Orient& b)
{
    Orient r{};
    for (int k = 0; k < 3; ++k) {
        r.axis[k] = a.axis[b.axis[k]];
        r.flip |= (((b.flip >> k) ^ (a.flip >> b.axis[k])) & 1u) << k;
    }
    return r;
}

inline Orient orient_inverse(const Orient& o)
{
    Orient r{};
    for (int k = 0; k < 3; ++k) {
        r.axis[o.axis[k]] = k;
        r.flip |= ((o.flip >> k) & 1u) << o.axis[k];
    }
    return r;
}

// right-handed quarter turns about `axis`: one turn takes axis a + 1 onto a + 2 (mod 3).  false for an axis outside 0 .. 2.
inline bool orient_rotation(int axis, int quarter_turns, Orient& out)
{
    if (axis < 0 || axis > 2)
        return false;
    const int b = (axis + 1) % 3, c = (axis + 2) % 3;
    Orient q{};  // one turn: q[a] = p[a], q[c] = p[b], q[b] = sd[c] - 1 - p[c]
    q.axis[axis] = axis;
    q.axis[b] = c;
    q.axis[c] = b;
    q.flip = 1u << b;
    out = Orient{{0, 1, 2}, 0u};
    for (int n = ((quarter_turns % 4) + 4) % 4; n > 0; --n)
        out = orient_compose(out, q);
    return true;
}

inline void orient_dims(const Orient& o, const int32_t sd[3], int32_t dd[3])
{
    const int32_t s[3] = {sd[0], sd[1], sd[2]};  // (dd may be sd)
    for (int k = 0; k < 3; ++k)
        dd[k] = s[o.axis[k]];
}

inline void orient_voxel(const Orient& o, const int32_t sd[3], const int32_t p[3], int32_t q[3])
{
    const int32_t s[3] = {p[0], p[1], p[2]};
    for (int k = 0; k < 3; ++k)
        q[k] = ((o.flip >> k) & 1u) ? sd[o.axis[k]] - 1 - s[o.axis[k]] : s[o.axis[k]];
}

// the sign of the permutation times (-1)^popcount(flip) is +1
inline bool orient_is_rotation(const Orient& o)
{
    const bool even = (o.axis[0] == 0 && o.axis[1] == 1) || (o.axis[0] == 1 && o.axis[1] == 2) || (o.axis[0] == 2 && o.axis[1] == 0);
    return even == ((__builtin_popcount(o.flip) & 1) == 0);
}

// ---- the plan of a call ----------------------------------------------------------------------------------------------------
struct TransformArgs {
    const uint32_t* src;
    uint32_t* dst;
    uint32_t* summary;  // vxrt_transform_summary as words, or NULL
    int32_t sd[3], dd[3], axis[3];
    uint32_t flip;
    uint32_t wps, wpd;    // words per source row, per destination row
    uint64_t nsrc, ndst;  // words (at most 2^31: a word index fits 32 bits, a byte offset does not)
    // COPY class
    uint32_t c1, c2;      // the source word strides of destination axes 1 and 2
    TrDiv by_wpd, by_dd1;
    // TRANSPOSE class
    int32_t s, t;         // the source axis along destination x, and the third source axis
    int32_t kx, kt;       // the destination axes of source x and of source t (1 or 2)
    uint32_t ss, st;      // the source word strides of axes s and t
    uint32_t dx, dt;      // the destination word strides of the axes source x and t land on
    uint32_t tiles_j, tiles_x;
    uint64_t tiles;       // tiles_j * tiles_x * sd[t]
    TrDiv by_tiles_x, by_tiles_j;
};

// 0 = inside the contract, 1 = bad dims, 2 = a word count beyond kTransformMaxWords; fills everything but the pointers
inline int transform_plan(const int32_t sd[3], const Orient& o, TransformArgs& A)
{
    A = TransformArgs{};
    if (region_words(sd) == 0)
        return 1;
    for (int k = 0; k < 3; ++k) {
        A.sd[k] = sd[k];
        A.axis[k] = o.axis[k];
        A.dd[k] = sd[o.axis[k]];
    }
    A.flip = o.flip;
    A.nsrc = region_words(A.sd);
    A.ndst = region_words(A.dd);  // (the same voxels: never 0)
    if (A.nsrc > kTransformMaxWords || A.ndst > kTransformMaxWords)
        return 2;
    A.wps = (uint32_t)region_words_per_row(A.sd[0]);
    A.wpd = (uint32_t)region_words_per_row(A.dd[0]);
    const uint32_t srow[3] = {0u, A.wps, (uint32_t)A.sd[1] * A.wps}, drow[3] = {0u, A.wpd, (uint32_t)A.dd[1] * A.wpd};  // (below 2^31)
    if (A.axis[0] == 0) {
        A.c1 = srow[A.axis[1]];
        A.c2 = srow[A.axis[2]];
        A.by_wpd = tr_div_by(A.wpd);
        A.by_dd1 = tr_div_by((uint32_t)A.dd[1]);
    } else {
        A.s = A.axis[0];
        A.t = 3 - A.s;
        A.kx = A.axis[1] == 0 ? 1 : 2;
        A.kt = 3 - A.kx;
        A.tiles_j = (A.wpd + kTrTJ - 1u) / kTrTJ;
        A.tiles_x = (A.wps + kTrTX - 1u) / kTrTX;
        A.tiles = (uint64_t)A.tiles_j * A.tiles_x * (uint64_t)A.sd[A.t];  // at most the source's words
        A.ss = srow[A.s];
        A.st = srow[A.t];
        A.dx = drow[A.kx];
        A.dt = drow[A.kt];
        A.by_tiles_x = tr_div_by(A.tiles_x);
        A.by_tiles_j = tr_div_by(A.tiles_j);
    }
    return 0;
}

// the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool transform_overlap(const void* a, uint64_t na, const void* b, uint64_t nb)
{
    const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
    return x < y + nb && y < x + na;
}

// The checks of a call after the NULL ctx, in the order of include/vxrt.h: 0 = accepted (A filled, the summary apart),
// 1 = a NULL argument, 2 = an invalid orientation, 3 = bad dims, 4 = a word cap, 5 = the ranges overlap
inline int transform_check(const uint32_t* src, const int32_t* sd, const Orient* o, uint32_t* dst, TransformArgs& A)
{
    if (!src || !sd || !o || !dst)
        return 1;
    if (!orient_valid(*o))
        return 2;
    if (const int bad = transform_plan(sd, *o, A))
        return 2 + bad;
    if (transform_overlap(src, 4u * A.nsrc, dst, 4u * A.ndst))
        return 5;
    A.src = src;
    A.dst = dst;
    return 0;
}

// workgroups of the launch
inline uint32_t transform_groups(const TransformArgs& A)
{
    const uint64_t n = A.axis[0] == 0 ? (A.ndst + kTrLanes - 1u) / kTrLanes : A.tiles;
    return (uint32_t)(n < kTrMaxGroups ? n : kTrMaxGroups);
}

// ---- the per-lane work -------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t tr_brev(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// a lane's tally: the set voxels of the words it stored and their inclusive bounds in destination coordinates
struct TrTally {
    uint32_t n;
    int32_t lo[3], hi[3];
};

__host__ __device__ inline void tr_tally_clear(TrTally& t)
{
    t.n = 0u;
    for (int k = 0; k < 3; ++k) {
        t.lo[k] = INT32_MAX;
        t.hi[k] = INT32_MIN;
    }
}

// destination word j of destination row (q1, q2)
__host__ __device__ inline void tr_tally_word(TrTally& t, uint32_t word, uint32_t j, int32_t q1, int32_t q2)
{
    if (!word)
        return;
    t.n += (uint32_t)__builtin_popcount(word);
    const int32_t x0 = (int32_t)(32u * j) + __builtin_ctz(word), x1 = (int32_t)(32u * j) + 31 - __builtin_clz(word);
    const int32_t lo[3] = {x0, q1, q2}, hi[3] = {x1, q1, q2};
    for (int k = 0; k < 3; ++k) {
        t.lo[k] = lo[k] < t.lo[k] ? lo[k] : t.lo[k];
        t.hi[k] = hi[k] > t.hi[k] ? hi[k] : t.hi[k];
    }
}

// word `i` of the summary before the launch: no voxel, the bounds INT32_MAX / INT32_MIN
__host__ __device__ inline uint32_t tr_summary_init(uint32_t i)
{
    return i < kTrSumMin ? 0u : (i < kTrSumMax ? (uint32_t)INT32_MAX : (uint32_t)INT32_MIN);
}

// COPY class: destination word w computed, stored and tallied.  Word indices in 32 bits, the addresses in 64.
__host__ __device__ inline void tr_copy_word(const TransformArgs& A, uint32_t w, bool tally, TrTally& t)
{
    const uint32_t row = tr_div(w, A.by_wpd), j = w - row * A.wpd;
    const uint32_t q2 = tr_div(row, A.by_dd1), q1 = row - q2 * (uint32_t)A.dd[1];
    const uint32_t p1 = (A.flip & 2u) ? (uint32_t)A.dd[1] - 1u - q1 : q1, p2 = (A.flip & 4u) ? (uint32_t)A.dd[2] - 1u - q2 : q2;
    const uint32_t base = p1 * A.c1 + p2 * A.c2;
    uint32_t word;
    if (A.flip & 1u) {
        const int64_t sx = (int64_t)A.sd[0] - 32 * ((int64_t)j + 1), k = sx >> 5;
        if (k >= 0)  // (k < wps always: sx + 31 <= sd[0] - 1)
            VXRT_TRANSFORM_CHECK(kTrSrc, (uint64_t)base + (uint64_t)k);
        if (k + 1 >= 0 && (uint64_t)(k + 1) < A.wps)
            VXRT_TRANSFORM_CHECK(kTrSrc, (uint64_t)base + (uint64_t)(k + 1));
        word = tr_brev(row_gather32(A.src + (size_t)base, A.wps, sx));
    } else {
        VXRT_TRANSFORM_CHECK(kTrSrc, (uint64_t)base + j);
        word = A.src[(size_t)base + j];
        if (j == A.wps - 1u)
            word &= row_last_mask(A.sd[0]);
    }
    VXRT_TRANSFORM_CHECK(kTrDst, w);
    A.dst[(size_t)w] = word;
    if (tally)
        tr_tally_word(t, word, j, (int32_t)q1, (int32_t)q2);
}

// TRANSPOSE class: where a tile lies
struct TrTile {
    uint32_t j0, xw0;      // its first destination word and its first source x-word
    int32_t pt, qt;        // its coordinate on the third source axis, and where that lands
    uint32_t sbase, dbase; // the word offsets of pt in the source and of qt in the destination
};

__host__ __device__ inline TrTile tr_tile(const TransformArgs& A, uint32_t tile)
{
    TrTile T;
    const uint32_t a = tr_div(tile, A.by_tiles_x), pt = tr_div(a, A.by_tiles_j);
    T.xw0 = (tile - a * A.tiles_x) * kTrTX;
    T.j0 = (a - pt * A.tiles_j) * kTrTJ;
    T.pt = (int32_t)pt;
    T.qt = ((A.flip >> A.kt) & 1u) ? A.sd[A.t] - 1 - T.pt : T.pt;
    T.sbase = pt * A.st;
    T.dbase = (uint32_t)T.qt * A.dt;
    return T;
}

// element e of lane `lane` in the load phase: row r of the tile (along s) and x-word xl of the tile
__host__ __device__ inline void tr_load_slot(uint32_t lane, uint32_t e, uint32_t& r, uint32_t& xl)
{
    const uint32_t id = e * kTrLanes + lane;
    r = id / kTrTX;
    xl = id % kTrTX;
}

__host__ __device__ inline uint32_t tr_lds_in(uint32_t r, uint32_t xl) { return r * kTrPitchIn + xl; }
__host__ __device__ inline uint32_t tr_lds_out(uint32_t xrow, uint32_t jl) { return xrow * kTrPitchOut + jl; }

// the source word of row r, x-word xl of the tile: 0 outside the source, the bits beyond sd[0] cleared
__host__ __device__ inline uint32_t tr_load_word(const TransformArgs& A, const TrTile& T, uint32_t r, uint32_t xl)
{
    const uint32_t j = T.j0 + (r >> 5), xw = T.xw0 + xl, S = (uint32_t)A.sd[A.s];
    // the row along s: a row below 0 (flipped x, the last word) wraps to a value beyond S
    const uint32_t ps = ((A.flip & 1u) ? S - 32u * (j + 1u) : 32u * j) + (r & 31u);
    if (j >= A.wpd || xw >= A.wps || ps >= S)
        return 0u;
    const uint32_t i = ps * A.ss + T.sbase + xw;
    VXRT_TRANSFORM_CHECK(kTrSrc, i);
    const uint32_t word = A.src[(size_t)i];
    return xw == A.wps - 1u ? word & row_last_mask(A.sd[0]) : word;
}

// block b of half-wave `half` (0 .. 7) in the transpose phase: destination word jl and x-word xl of the tile
__host__ __device__ inline void tr_block(uint32_t half, uint32_t b, uint32_t& jl, uint32_t& xl)
{
    const uint32_t id = b * (kTrLanes / 32u) + half;
    jl = id / kTrTX;
    xl = id % kTrTX;
}

// one butterfly round of one lane: round 0 .. 4 exchanges with the lane 16, 8, 4, 2, 1 away.  The lane without the
// partner's bit keeps its low fields and takes the partner's low fields as its high ones; the other lane the reverse.
__host__ __device__ inline uint32_t tr_combine(uint32_t own, uint32_t partner, uint32_t round, uint32_t lane)
{
    const uint32_t m = 16u >> round;
    const uint32_t mask = round == 0u ? 0x0000FFFFu : round == 1u ? 0x00FF00FFu : round == 2u ? 0x0F0F0F0Fu : round == 3u ? 0x33333333u : 0x55555555u;
    return (lane & m) ? (own & ~mask) | ((partner >> m) & mask) : (own & mask) | ((partner << m) & ~mask);
}

// the transposed word as the destination holds it: bit-reversed where destination x runs against s
__host__ __device__ inline uint32_t tr_finish_word(const TransformArgs& A, uint32_t word) { return (A.flip & 1u) ? tr_brev(word) : word; }

// element e of lane `lane` in the store phase: destination row xrow of the tile (along source x) and word jl of the tile
__host__ __device__ inline void tr_store_slot(uint32_t lane, uint32_t e, uint32_t& xrow, uint32_t& jl)
{
    const uint32_t id = e * kTrLanes + lane;
    xrow = id / kTrTJ;
    jl = id % kTrTJ;
}

// the word of destination row xrow, word jl of the tile stored and tallied; nothing beyond the destination
__host__ __device__ inline void tr_store_word(const TransformArgs& A, const TrTile& T, uint32_t xrow, uint32_t jl, uint32_t word,
                                              bool tally, TrTally& t)
{
    const uint32_t j = T.j0 + jl, x = 32u * T.xw0 + xrow;
    if (j >= A.wpd || x >= (uint32_t)A.sd[0])
        return;
    const uint32_t qx = ((A.flip >> A.kx) & 1u) ? (uint32_t)A.sd[0] - 1u - x : x;
    const uint32_t i = qx * A.dx + T.dbase + j;
    VXRT_TRANSFORM_CHECK(kTrDst, i);
    A.dst[(size_t)i] = word;
    if (tally)
        tr_tally_word(t, word, j, A.kx == 1 ? (int32_t)qx : T.qt, A.kx == 1 ? T.qt : (int32_t)qx);
}

// a workgroup's tally into the summary: one atomic add, and a minimum or maximum only where the bound it read is not
// already as wide (the bounds only ever widen, so a stale read costs an atomic, never a result); nothing for a workgroup
// without a set voxel
__host__ __device__ inline void tr_commit(const TransformArgs& A, uint64_t n, const int32_t lo[3], const int32_t hi[3])
{
    if (!n)
        return;
    VXRT_TRANSFORM_CHECK(kTrSum, 1u);
    atom_add64((uint64_t*)A.summary, n);
    int32_t* box = (int32_t*)A.summary;
    for (uint32_t k = 0; k < 3u; ++k) {
        VXRT_TRANSFORM_CHECK(kTrSum, kTrSumMax + k);
        if ((int32_t)atom_load(A.summary + kTrSumMin + k) > lo[k])
            atom_min(box + kTrSumMin + k, lo[k]);
        if ((int32_t)atom_load(A.summary + kTrSumMax + k) < hi[k])
            atom_max(box + kTrSumMax + k, hi[k]);
    }
}

#ifndef VXRT_HOST_CHECK  // the launches of vxrt_transform.hip; A from transform_plan, the pointers set
hipError_t transform_stamp(const TransformArgs& A, hipStream_t stream);
#endif

}  // namespace vxrt
