// vxrt_loose.hpp -- loose voxels (include/vxrt.h, vxrt_loose_step): the pieces shared by the kernels of vxrt_loose.hip, the host
// side in vxrt_api_query.hip and the host harness of the tests (tests/tools/loose_check.cpp, through tests/tools/hoststub):
// the checks of the parameters, the workspace layout and, one lane at a time, the work of every launch.
//
// Halo.  h = 1: halo voxel (hx, hy, hz) is world voxel origin - 1 + (hx, hy, hz), so voxel (x, y, z) of B is halo voxel
// (x + 1, y + 1, z + 1).  A PLANE is one bit per halo voxel in vxrt_read_region's layout (wh words per row, word
// xw + wh * (hy + h[1] * hz), a row's padding bits 0 in every plane).  Four planes: BLOCKED (the halo's solid bits from
// k_read_region; under VXRT_LOOSE_WALL every voxel outside Live as well), LIVE (B intersected with the world) and two planes
// that hold the layer L and that the passes write in turn.  A halo voxel that is neither blocked nor live is a sink: L is
// never set there, so free = ~(blocked | L) holds for it as for every other voxel.
// Pass.  One lane per plane word.  With O = blocked | L ("occupied") and rows named by their (y, z):
//   FALL    movers   = L(y) & ~O(y-1);                                   arrivals = L(y+1) & ~O(y)
//   SLIDE   movers   = L(y) & O(y-1) & ~O(y)[at +d] & ~O(y-1)[at +d];    arrivals = (L(y+1) & O(y))[from -d'] & ~O(y+1) & ~O(y)
//   SPREAD  movers   = L(y) & O(y-1) & ~O(y)[at +d];                     arrivals = (L(y) & O(y-1))[from -d] & ~O(y)
//   new = (L & ~movers) | (arrivals & live)
// d is the direction of the voxel itself, d' of the voxel one row up: along x it is one direction per row (the word shifted
// one voxel with the carry bit of the neighbouring word), along z one direction per bit, selected by 0x55555555 or its
// complement out of the rows z - 1 and z + 1.  A row or a word outside the halo box holds nothing and is not loaded.
// Output.  One lane per word of d_loose_out: the 32 voxels funnel-shifted out of L_n and the blocked plane (B's words sit at
// bit offset 1 in the halo's), cut to the world voxels of B, compared with the input word of the same index (read before
// the store: the two may be one buffer), stored and tallied.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into a plane, the input, the output or the summary against
// that array's size (array: one of the kLoose* ids below).  The kernels leave it empty.
#ifndef VXRT_LOOSE_CHECK
#define VXRT_LOOSE_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint64_t kLooseMaxVoxels = 1ull << 28;
constexpr int32_t kLooseMaxSteps = 64;
enum { kLooseSand = 0, kLooseWater = 1 };
enum { kLooseWall = 0, kLooseOpen = 1 };
enum { kLoosePlane, kLooseIn, kLooseOut, kLooseSummary };
enum { kLooseFall = 0, kLooseSlide = 1, kLooseSpread = 2 };
// summary words (vxrt_loose_summary)
enum {
    kLooseSumIn = 0, kLooseSumStart = 1, kLooseSumAfter = 2, kLooseSumFell = 3, kLooseSumSlid = 4, kLooseSumSpread = 5,
    kLooseSumMin = 6, kLooseSumMax = 9, kLooseSumWords = 12
};

// 0 when the parameters are within the contract, else the number of the first check they fail, in the order of
// include/vxrt.h: 1 struct_size, 2 material, 3 steps, 4 edge, 5 reserved_
inline int loose_check(const vxrt_loose& p)
{
    if (p.struct_size != sizeof(vxrt_loose))
        return 1;
    if (p.material != kLooseSand && p.material != kLooseWater)
        return 2;
    if (p.steps < 1 || p.steps > kLooseMaxSteps)
        return 3;
    if (p.edge != kLooseWall && p.edge != kLooseOpen)
        return 4;
    if (p.reserved_[0] != 0 || p.reserved_[1] != 0 || p.reserved_[2] != 0)
        return 5;
    return 0;
}

// passes of a step, and of a call
inline int32_t loose_passes_per_step(int32_t material) { return material == kLooseWater ? 3 : 2; }
inline int32_t loose_passes(const vxrt_loose& p) { return p.steps * loose_passes_per_step(p.material); }

// the workspace: four planes, each on a 256-byte boundary (include/vxrt.h states the same formula)
struct LooseLayout : HaloBox {       // the halo box (vxrt_region.hpp): B grown by 1
    uint64_t blocked, live, turn[2];  // byte offsets
    uint64_t total_bytes;
    uint64_t np, nb;  // words of a plane (= nhalo), of the layer in B's region layout
    uint32_t mw;      // words per row of the layer
};

// false outside the contract (L.fault: why): dims, the halo box within a region read and, when `o` is given, within int32
inline bool loose_layout(const int32_t* o, const int32_t d[3], LooseLayout& L)
{
    L.fault = halo_box(o, d, 1, kLooseMaxVoxels, L);
    if (L.fault != kBoxOk)
        return false;
    L.np = L.nhalo;
    L.nb = region_words(d);
    L.mw = (uint32_t)region_words_per_row(d[0]);
    Sections S;
    L.blocked = S.take(4u * L.np);
    L.live = S.take(4u * L.np);
    L.turn[0] = S.take(4u * L.np);
    L.turn[1] = S.take(4u * L.np);
    L.total_bytes = S.at;
    return true;
}

// what the loose kernels read and write (device pointers; host pointers in the harness)
struct LooseArgs {
    uint32_t* blocked;   // over the halo box
    uint32_t* live;      // over the halo box
    uint32_t* turn[2];   // pass p (0 ..) reads turn[p & 1] and writes turn[(p + 1) & 1]
    const uint32_t* in;  // the input layer, B's region layout
    uint32_t* out;       // the output layer; may be `in`
    uint32_t* summary;   // output: vxrt_loose_summary
    uint64_t np, nb;
    int32_t o[3], d[3];
    int32_t dim[3];  // world voxels per axis
    uint32_t wh, hy, hz, mw;
    int32_t edge;
};

inline void loose_args(LooseArgs& A, const LooseLayout& L, const CollideWorld& W, const int32_t o[3], const int32_t d[3],
                       const vxrt_loose& p, const uint32_t* in, void* work, uint32_t* out, uint32_t* summary)
{
    char* w = (char*)work;
    A.blocked = (uint32_t*)(w + L.blocked);
    A.live = (uint32_t*)(w + L.live);
    A.turn[0] = (uint32_t*)(w + L.turn[0]);
    A.turn[1] = (uint32_t*)(w + L.turn[1]);
    A.in = in;
    A.out = out;
    A.summary = summary;
    A.np = L.np;
    A.nb = L.nb;
    for (int k = 0; k < 3; ++k) {
        A.o[k] = o[k];
        A.d[k] = d[k];
        A.dim[k] = W.dim[k];
    }
    A.wh = L.wh;
    A.hy = L.hy;
    A.hz = L.hz;
    A.mw = L.mw;
    A.edge = p.edge;
}

// pass p of a call (0 ..): which pass of its step, the step's number t, the plane it reads and the plane it writes
inline int loose_pass_kind(int32_t material, int32_t p) { return p % loose_passes_per_step(material); }
inline uint32_t loose_pass_step(const vxrt_loose& q, int32_t p) { return q.phase + (uint32_t)(p / loose_passes_per_step(q.material)); }
inline const uint32_t* loose_src(const LooseArgs& A, int32_t p) { return A.turn[p & 1]; }
inline uint32_t* loose_dst(const LooseArgs& A, int32_t p) { return A.turn[(p + 1) & 1]; }

// the bits j of a word whose voxel x0 + j lies in [lo, hi]
__host__ __device__ inline uint32_t loose_span(int64_t x0, int64_t lo, int64_t hi)
{
    const int64_t a = lo - x0 < 0 ? 0 : lo - x0, b = hi - x0 > 31 ? 31 : hi - x0;
    return a > b ? 0u : bit_range((int)a, (int)b);
}

// the 32 bits sx .. sx + 31 of one row of `nw` words of array `array` (row_gather32 with every index checked)
__host__ __device__ inline uint32_t loose_gather(int array, const uint32_t* base, uint64_t row, uint64_t nw, int64_t sx)
{
    const int64_t k = sx >> 5;
    const int s = (int)(sx & 31);
    uint32_t lo = 0u, hi = 0u;
    if (k >= 0 && (uint64_t)k < nw) {
        VXRT_LOOSE_CHECK(array, row + (uint64_t)k);
        lo = base[row + (uint64_t)k];
    }
    if (s && k + 1 >= 0 && (uint64_t)(k + 1) < nw) {
        VXRT_LOOSE_CHECK(array, row + (uint64_t)(k + 1));
        hi = base[row + (uint64_t)(k + 1)];
    }
    (void)array;
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> s);
}

// ---- k_loose_setup: lane i = plane word ---------------------------------------------------------------------------------------
// the value lane i < kLooseSumWords gives summary word i before anything is tallied
__host__ __device__ inline uint32_t loose_summary_init(uint32_t i)
{
    return i >= kLooseSumMax ? (uint32_t)INT32_MIN : i >= kLooseSumMin ? (uint32_t)INT32_MAX : 0u;
}

// the blocked word completed (under VXRT_LOOSE_WALL everything outside Live set), the live word built and L_start's word
// written to turn[0]: the input funnel-shifted to bit offset 1, cut to Live & ~blocked
__host__ __device__ inline void loose_setup_lane(const LooseArgs& A, uint64_t i)
{
    const uint32_t xw = (uint32_t)(i % A.wh);
    const uint64_t row = i / A.wh;
    const uint32_t y = (uint32_t)(row % A.hy), z = (uint32_t)(row / A.hy);
    const int64_t x0 = (int64_t)A.o[0] - 1 + 32 * (int64_t)xw, wy = (int64_t)A.o[1] - 1 + y, wz = (int64_t)A.o[2] - 1 + z;
    const uint32_t rmask = loose_span(32 * (int64_t)xw, 0, (int64_t)A.d[0] + 1);
    const bool yz_live = wy >= 0 && wy < A.dim[1] && wz >= 0 && wz < A.dim[2] && y >= 1u && y <= (uint32_t)A.d[1] && z >= 1u &&
                         z <= (uint32_t)A.d[2];
    const uint32_t live = yz_live ? loose_span(x0, 0, (int64_t)A.dim[0] - 1) & loose_span(32 * (int64_t)xw, 1, (int64_t)A.d[0]) : 0u;
    VXRT_LOOSE_CHECK(kLoosePlane, i);
    uint32_t blocked = A.blocked[i];
    if (A.edge == kLooseWall)
        blocked |= rmask & ~live;
    A.blocked[i] = blocked;
    A.live[i] = live;
    uint32_t l = 0u;
    if (live & ~blocked) {
        const uint64_t irow = ((uint64_t)(y - 1u) + (uint64_t)A.d[1] * (z - 1u)) * A.mw;
        l = loose_gather(kLooseIn, A.in, irow, A.mw, 32 * (int64_t)xw - 1) & live & ~blocked;
    }
    A.turn[0][i] = l;
}

// ---- k_loose_pass: lane i = plane word ---------------------------------------------------------------------------------------
// one word of a plane, 0 and not loaded when the row lies outside the halo box
__host__ __device__ inline uint32_t loose_word(const uint32_t* plane, int64_t w, bool in)
{
    if (!in)
        return 0u;
    VXRT_LOOSE_CHECK(kLoosePlane, (uint64_t)w);
    return plane[w];
}

// bit j = the voxel at x - 1 (`up`) or at x + 1 of the row of word w, whose value is c: the word shifted one voxel with the
// carry bit of the neighbouring word; nothing comes in across the ends of a row
__host__ __device__ inline uint32_t loose_shift(const LooseArgs& A, const uint32_t* plane, int64_t w, uint32_t xw, uint32_t c, bool up)
{
    if (up)
        return c << 1 | (xw > 0u ? loose_word(plane, w - 1, true) >> 31 : 0u);
    return c >> 1 | (xw + 1u < A.wh ? loose_word(plane, w + 1, true) << 31 : 0u);
}

// The new word i of L after pass PASS of step t, from the plane `src` that holds L before it; *moved: the word's movers.
// SHORTCUT: a word that holds nothing and that nothing can arrive in is 0 without a look at the blocked plane.
template <int PASS, bool SHORTCUT>
__host__ __device__ inline uint32_t loose_pass_word(const LooseArgs& A, const uint32_t* src, uint64_t i, uint32_t t, uint32_t* moved)
{
    const uint32_t xw = (uint32_t)(i % A.wh);
    const uint64_t row = i / A.wh;
    const uint32_t y = (uint32_t)(row % A.hy), z = (uint32_t)(row / A.hy);
    const int64_t sy = (int64_t)A.wh, sz = (int64_t)A.wh * (int64_t)A.hy, w = (int64_t)i;
    const bool dn = y > 0u, up = y + 1u < A.hy, zl = z > 0u, zh = z + 1u < A.hz;
    const uint32_t* B = A.blocked;
    *moved = 0u;
    VXRT_LOOSE_CHECK(kLoosePlane, i);
    const uint32_t l = src[i];
    if (PASS == kLooseFall) {
        const uint32_t la = loose_word(src, w + sy, up);
        if (SHORTCUT && !(l | la))
            return 0u;
        const uint32_t ob = dn ? loose_word(src, w - sy, true) | loose_word(B, w - sy, true) : 0xFFFFFFFFu;
        const uint32_t o = l | loose_word(B, w, true);
        const uint32_t movers = l & ~ob;
        *moved = movers;
        return (l & ~movers) | (la & ~o & loose_word(A.live, w, true));
    }
    // the parity term of the direction that this row's voxels share: world y + (t >> 1); one row up it is the other
    const uint32_t py = ((uint32_t)A.o[1] - 1u + y + (t >> 1)) & 1u;
    if ((t & 1u) == 0u) {
        // along x: s = (world z + world y + (t >> 1)) & 1 for the whole row; 0: towards +x
        const bool minus = ((((uint32_t)A.o[2] - 1u + z) & 1u) ^ py) != 0u;
        if (PASS == kLooseSlide) {
            // arrivals come from the row above, whose direction is the other one: towards +x, from x - 1, when this row
            // moves towards -x; la_n: the word of that row whose carry bit can arrive here
            const uint32_t la = loose_word(src, w + sy, up);
            const uint32_t la_n = up ? (minus ? (xw > 0u ? loose_word(src, w + sy - 1, true) : 0u)
                                             : (xw + 1u < A.wh ? loose_word(src, w + sy + 1, true) : 0u)) : 0u;
            if (SHORTCUT && !(l | la | la_n))
                return 0u;
            const uint32_t b = loose_word(B, w, true), o = l | b;
            const uint32_t lb = loose_word(src, w - sy, dn), bb = dn ? loose_word(B, w - sy, true) : 0xFFFFFFFFu, ob = lb | bb;
            // movers: resting, the voxel beside and the voxel beside and below free
            const uint32_t o_side = loose_shift(A, src, w, xw, l, minus) | loose_shift(A, B, w, xw, b, minus);
            const uint32_t ob_side = dn ? loose_shift(A, src, w - sy, xw, lb, minus) | loose_shift(A, B, w - sy, xw, bb, minus)
                                        : 0xFFFFFFFFu;
            const uint32_t movers = l & ob & ~o_side & ~ob_side;
            // arrivals: the resting voxels of the row above, moved one voxel along their direction
            uint32_t arrive = 0u;
            if (up) {
                const uint32_t oa = la | loose_word(B, w + sy, true);
                // resting in the row above: on this row's occupied voxels
                const uint32_t rest_a = la & o;
                // the same one voxel to the side, from the neighbouring word's carry bit: its resting bit
                uint32_t carry = 0u;
                if (minus && xw > 0u)  // the row above moves towards +x: the source is at x - 1
                    carry = (loose_word(src, w + sy - 1, true) & (loose_word(src, w - 1, true) | loose_word(B, w - 1, true))) >> 31;
                if (!minus && xw + 1u < A.wh)  // the row above moves towards -x: the source is at x + 1
                    carry = (loose_word(src, w + sy + 1, true) & (loose_word(src, w + 1, true) | loose_word(B, w + 1, true))) << 31;
                const uint32_t from = (minus ? rest_a << 1 : rest_a >> 1) | carry;
                arrive = from & ~oa & ~o;
            }
            *moved = movers;
            return (l & ~movers) | (arrive & loose_word(A.live, w, true));
        }
        // SPREAD along x: sources in this row, one voxel against the direction
        const uint32_t l_n = minus ? (xw + 1u < A.wh ? loose_word(src, w + 1, true) : 0u) : (xw > 0u ? loose_word(src, w - 1, true) : 0u);
        if (SHORTCUT && !(l | l_n))
            return 0u;
        const uint32_t b = loose_word(B, w, true), o = l | b;
        const uint32_t ob = dn ? loose_word(src, w - sy, true) | loose_word(B, w - sy, true) : 0xFFFFFFFFu;
        const uint32_t rest = l & ob;
        const uint32_t o_side = loose_shift(A, src, w, xw, l, minus) | loose_shift(A, B, w, xw, b, minus);
        const uint32_t movers = rest & ~o_side;
        uint32_t carry = 0u;
        if (!minus && xw > 0u)
            carry = (l_n & (dn ? loose_word(src, w - sy - 1, true) | loose_word(B, w - sy - 1, true) : 0xFFFFFFFFu)) >> 31;
        if (minus && xw + 1u < A.wh)
            carry = (l_n & (dn ? loose_word(src, w - sy + 1, true) | loose_word(B, w - sy + 1, true) : 0xFFFFFFFFu)) << 31;
        const uint32_t from = (minus ? rest >> 1 : rest << 1) | carry;
        *moved = movers;
        return (l & ~movers) | (from & ~o & loose_word(A.live, w, true));
    }
    // along z: s = (world x + world y + (t >> 1)) & 1 per bit; `plus`: the bits of this row whose voxels move towards +z
    const uint32_t plus = ((((uint32_t)A.o[0] - 1u) & 1u) ^ py) ? 0xAAAAAAAAu : 0x55555555u;
    if (PASS == kLooseSlide) {
        // arrivals: from the row above at z - 1 moving towards +z (its plus bits are ~plus), at z + 1 moving towards -z
        const uint32_t la_l = loose_word(src, w + sy - sz, up && zl), la_h = loose_word(src, w + sy + sz, up && zh);
        if (SHORTCUT && !(l | la_l | la_h))
            return 0u;
        const uint32_t o = l | loose_word(B, w, true);
        const uint32_t ob = dn ? loose_word(src, w - sy, true) | loose_word(B, w - sy, true) : 0xFFFFFFFFu;
        const uint32_t o_l = zl ? loose_word(src, w - sz, true) | loose_word(B, w - sz, true) : 0xFFFFFFFFu;
        const uint32_t o_h = zh ? loose_word(src, w + sz, true) | loose_word(B, w + sz, true) : 0xFFFFFFFFu;
        const uint32_t ob_l = dn && zl ? loose_word(src, w - sy - sz, true) | loose_word(B, w - sy - sz, true) : 0xFFFFFFFFu;
        const uint32_t ob_h = dn && zh ? loose_word(src, w - sy + sz, true) | loose_word(B, w - sy + sz, true) : 0xFFFFFFFFu;
        const uint32_t movers = l & ob & ((plus & ~o_h & ~ob_h) | (~plus & ~o_l & ~ob_l));
        uint32_t arrive = 0u;
        if (up) {
            const uint32_t oa = loose_word(src, w + sy, true) | loose_word(B, w + sy, true);
            arrive = ((la_l & o_l & ~plus) | (la_h & o_h & plus)) & ~oa & ~o;
        }
        *moved = movers;
        return (l & ~movers) | (arrive & loose_word(A.live, w, true));
    }
    // SPREAD along z: sources in the rows z - 1 (moving towards +z) and z + 1 (towards -z) of this y
    const uint32_t l_l = loose_word(src, w - sz, zl), l_h = loose_word(src, w + sz, zh);
    if (SHORTCUT && !(l | l_l | l_h))
        return 0u;
    const uint32_t o = l | loose_word(B, w, true);
    const uint32_t ob = dn ? loose_word(src, w - sy, true) | loose_word(B, w - sy, true) : 0xFFFFFFFFu;
    const uint32_t o_l = zl ? l_l | loose_word(B, w - sz, true) : 0xFFFFFFFFu;
    const uint32_t o_h = zh ? l_h | loose_word(B, w + sz, true) : 0xFFFFFFFFu;
    const uint32_t ob_l = dn && zl ? loose_word(src, w - sy - sz, true) | loose_word(B, w - sy - sz, true) : 0xFFFFFFFFu;
    const uint32_t ob_h = dn && zh ? loose_word(src, w - sy + sz, true) | loose_word(B, w - sy + sz, true) : 0xFFFFFFFFu;
    const uint32_t movers = l & ob & ((plus & ~o_h) | (~plus & ~o_l));
    const uint32_t arrive = ((l_l & ob_l & plus) | (l_h & ob_h & ~plus)) & ~o;
    *moved = movers;
    return (l & ~movers) | (arrive & loose_word(A.live, w, true));
}

// returns the number of the word's movers
template <int PASS, bool SHORTCUT>
__host__ __device__ inline uint32_t loose_pass_lane(const LooseArgs& A, const uint32_t* src, uint32_t* dst, uint64_t i, uint32_t t)
{
    uint32_t moved;
    dst[i] = loose_pass_word<PASS, SHORTCUT>(A, src, i, t, &moved);
    return (uint32_t)__builtin_popcount(moved);
}

// ---- k_loose_output: lane i = word of the layer, xb + mw * (y + dims[1] * z) ----------------------------------------------------
// the tally of one lane, wave and workgroup: at most 2^28 voxels in all, so every count fits 32 bits
struct LooseTally {
    uint32_t n[3];  // loose_in, loose_start, loose_after
    int32_t lo[3], hi[3];
};

__host__ __device__ inline void loose_tally_clear(LooseTally& t)
{
    for (int k = 0; k < 3; ++k) {
        t.n[k] = 0u;
        t.lo[k] = INT32_MAX;
        t.hi[k] = INT32_MIN;
    }
}

// `last`: the plane that holds L_n
__host__ __device__ inline void loose_output_lane(const LooseArgs& A, const uint32_t* last, uint64_t i, LooseTally& t)
{
    const uint32_t xb = (uint32_t)(i % A.mw);
    const uint64_t row = i / A.mw;
    const uint32_t y = (uint32_t)(row % (uint32_t)A.d[1]), z = (uint32_t)(row / (uint32_t)A.d[1]);
    const int64_t x0 = (int64_t)A.o[0] + 32 * (int64_t)xb, wy = (int64_t)A.o[1] + y, wz = (int64_t)A.o[2] + z;
    const uint32_t valid = loose_span(32 * (int64_t)xb, 0, (int64_t)A.d[0] - 1);  // not padding
    // the input word first: the output may be the same buffer
    VXRT_LOOSE_CHECK(kLooseIn, i);
    const uint32_t win = A.in[i] & valid;
    const uint64_t hrow = (uint64_t)A.wh * ((uint64_t)(y + 1u) + (uint64_t)A.hy * (z + 1u));
    const int64_t sx = 32 * (int64_t)xb + 1;
    uint32_t wn = 0u, ws = 0u;
    if (wy >= 0 && wy < A.dim[1] && wz >= 0 && wz < A.dim[2]) {
        const uint32_t m = loose_span(x0, 0, (int64_t)A.dim[0] - 1) & valid;  // the world voxels of B in this word
        if (m) {
            wn = loose_gather(kLoosePlane, last, hrow, A.wh, sx) & m;
            if (win & m)
                ws = win & m & ~loose_gather(kLoosePlane, A.blocked, hrow, A.wh, sx);
        }
    }
    VXRT_LOOSE_CHECK(kLooseOut, i);
    A.out[i] = wn;
    t.n[0] += (uint32_t)__builtin_popcount(win);
    t.n[1] += (uint32_t)__builtin_popcount(ws);
    t.n[2] += (uint32_t)__builtin_popcount(wn);
    const uint32_t ch = wn ^ win;
    if (ch) {
        const int32_t xa = (int32_t)(x0 + __builtin_ctz(ch)), xz = (int32_t)(x0 + 31 - __builtin_clz(ch));
        t.lo[0] = xa < t.lo[0] ? xa : t.lo[0];
        t.hi[0] = xz > t.hi[0] ? xz : t.hi[0];
        t.lo[1] = (int32_t)wy < t.lo[1] ? (int32_t)wy : t.lo[1];
        t.hi[1] = (int32_t)wy > t.hi[1] ? (int32_t)wy : t.hi[1];
        t.lo[2] = (int32_t)wz < t.lo[2] ? (int32_t)wz : t.lo[2];
        t.hi[2] = (int32_t)wz > t.hi[2] ? (int32_t)wz : t.hi[2];
    }
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_loose.hip on the box o, d
hipError_t loose_step(const CollideWorld& W, const int32_t o[3], const int32_t d[3], const vxrt_loose& params, const uint32_t* loose_in,
                      void* work, uint32_t* loose_out, vxrt_loose_summary* summary, hipStream_t stream);
#endif

}  // namespace vxrt
