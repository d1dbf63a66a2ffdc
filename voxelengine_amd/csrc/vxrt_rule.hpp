// vxrt_rule.hpp -- neighbour-count voxel rules (include/vxrt.h, vxrt_apply_rule): the pieces shared by the kernels of
// vxrt_rule.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/rule_check.cpp, through
// tests/tools/hoststub): the checks of a rule, the workspace layout and, one lane at a time, the work of every launch.
//
// Halo.  h = 1 (VXRT_RULE_BOX) or `iterations` (VXRT_RULE_WORLD).  Halo voxel (hx, hy, hz) is world voxel origin - h +
// (hx, hy, hz), so voxel (x, y, z) of B is halo voxel (x + h, y + h, z + h).  A PLANE is one bit per halo voxel in
// vxrt_read_region's layout: wh = ceil((dims[0] + 2 h) / 32) words per row, word xw + wh * (hy + h[1] * hz), a row's padding
// bits 0 in every plane.  Four planes: W_0 (the halo's solid bits from k_read_region, the voxels outside the world set when
// `outside` is 1), F (the voxels a step may change) and two planes the rounds write in turn.
// Round.  One lane per plane word.  The nine rows (dy, dz) around the word each give a two-bit number per voxel, bit-sliced:
// a full row l + w + r (a full adder: l, r the word shifted one voxel each way with the carry bit of the neighbouring word),
// a row of which only w counts, or nothing; the centre row l + r.  A tree of bit-sliced adders sums the nine to the count in
// five planes, two mux trees over the count planes look the new bit up in `survive` and `born`, the word's own bits select
// between the two and F between the result and the word as it was.  A row or a word outside the halo box adds nothing: the
// region in which W_i is right shrinks by one voxel per round and still holds B after the last.
// Output.  One lane per word of d_bits: the 32 voxels funnel-shifted out of W_n, W_n-1 and W_0 (B's words sit at bit offset
// h < 32 in the halo's), cut to the world voxels of B, stored and tallied.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into a plane, the mask or the output against that array's
// size (array: one of the kRule* ids below).  The kernels leave it empty.
#ifndef VXRT_RULE_CHECK
#define VXRT_RULE_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint64_t kRuleMaxVoxels = 1ull << 28;
constexpr int32_t kRuleMaxIterations = 16;
enum { kRuleN6 = 0, kRuleN18 = 1, kRuleN26 = 2 };
enum { kRuleBox = 0, kRuleWorld = 1 };
enum { kRulePlane, kRuleMask, kRuleOut, kRuleSummary };
// summary words (vxrt_rule_summary)
enum {
    kRuleSumBefore = 0, kRuleSumAfter = 1, kRuleSumBorn = 2, kRuleSumDied = 3, kRuleSumLast = 4, kRuleSumMin = 6, kRuleSumMax = 9,
    kRuleSumWords = 12
};

// neighbours of a voxel in neighbourhood nb
constexpr uint32_t rule_neighbours(int32_t nb) { return nb == kRuleN6 ? 6u : nb == kRuleN18 ? 18u : 26u; }

// 0 when the rule's fields are within the contract, else the number of the first check it fails, in the order of
// include/vxrt.h: 1 struct_size, 2 neighbours, 3 bits of born or survive above N, 4 iterations, 5 scope, 6 outside, 7 reserved_
inline int rule_check(const vxrt_rule& r)
{
    if (r.struct_size != sizeof(vxrt_rule))
        return 1;
    if (r.neighbours < kRuleN6 || r.neighbours > kRuleN26)
        return 2;
    const uint32_t above = ~((2u << rule_neighbours(r.neighbours)) - 1u);
    if ((r.born | r.survive) & above)
        return 3;
    if (r.iterations < 1 || r.iterations > kRuleMaxIterations)
        return 4;
    if (r.scope != kRuleBox && r.scope != kRuleWorld)
        return 5;
    if (r.outside != 0 && r.outside != 1)
        return 6;
    if (r.reserved_ != 0)
        return 7;
    return 0;
}

// the halo of a checked rule
inline int32_t rule_halo(const vxrt_rule& r) { return r.scope == kRuleWorld ? r.iterations : 1; }

// the workspace: four planes, each on a 256-byte boundary (include/vxrt.h states the same formula)
struct RuleLayout : HaloBox {     // the halo box (vxrt_region.hpp): B grown by h
    uint64_t w0, free, turn[2];  // byte offsets
    uint64_t total_bytes;
    uint64_t np, nb;        // words of a plane (= nhalo), of d_bits
    uint32_t mw;            // words per row of d_bits and of the mask
    uint32_t h;
};

// false outside the contract (L.fault: why): dims, the halo box within a region read and, when `o` is given, within int32
// (h: rule_halo)
inline bool rule_layout(const int32_t* o, const int32_t d[3], int32_t h, RuleLayout& L)
{
    L.fault = h < 1 || h > kRuleMaxIterations ? kBoxDims : halo_box(o, d, h, kRuleMaxVoxels, L);
    if (L.fault != kBoxOk)
        return false;
    L.np = L.nhalo;
    L.nb = region_words(d);
    L.mw = (uint32_t)region_words_per_row(d[0]);
    L.h = (uint32_t)h;
    Sections S;
    L.w0 = S.take(4u * L.np);
    L.free = S.take(4u * L.np);
    L.turn[0] = S.take(4u * L.np);
    L.turn[1] = S.take(4u * L.np);
    L.total_bytes = S.at;
    return true;
}

// what the rule kernels read and write (device pointers; host pointers in the harness)
struct RuleArgs {
    uint32_t* w0;          // W_0 over the halo box
    uint32_t* free;        // F over the halo box
    uint32_t* turn[2];     // round i (0 ..) writes turn[i & 1]
    const uint32_t* mask;  // B's region layout, or NULL
    uint32_t* out;         // output: d_bits
    uint32_t* summary;     // output: vxrt_rule_summary
    uint64_t np, nb;
    int32_t o[3], d[3];
    int32_t dim[3];        // world voxels per axis
    uint32_t h, wh, hy, hz, mw;
    uint32_t born, survive;
    int32_t iterations, scope, outside;
};

inline void rule_args(RuleArgs& A, const RuleLayout& L, const CollideWorld& W, const int32_t o[3], const int32_t d[3],
                      const vxrt_rule& r, const uint32_t* mask, void* work, uint32_t* out, uint32_t* summary)
{
    char* w = (char*)work;
    A.w0 = (uint32_t*)(w + L.w0);
    A.free = (uint32_t*)(w + L.free);
    A.turn[0] = (uint32_t*)(w + L.turn[0]);
    A.turn[1] = (uint32_t*)(w + L.turn[1]);
    A.mask = mask;
    A.out = out;
    A.summary = summary;
    A.np = L.np;
    A.nb = L.nb;
    for (int k = 0; k < 3; ++k) {
        A.o[k] = o[k];
        A.d[k] = d[k];
        A.dim[k] = W.dim[k];
    }
    A.h = L.h;
    A.wh = L.wh;
    A.hy = L.hy;
    A.hz = L.hz;
    A.mw = L.mw;
    A.born = r.born;
    A.survive = r.survive;
    A.iterations = r.iterations;
    A.scope = r.scope;
    A.outside = r.outside;
}

// the plane round i reads, and the plane it writes
inline const uint32_t* rule_src(const RuleArgs& A, int32_t i) { return i == 0 ? A.w0 : A.turn[(i - 1) & 1]; }
inline uint32_t* rule_dst(const RuleArgs& A, int32_t i) { return A.turn[i & 1]; }

// the bits j of a word whose voxel x0 + j lies in [lo, hi]
__host__ __device__ inline uint32_t rule_span(int64_t x0, int64_t lo, int64_t hi)
{
    const int64_t a = lo - x0 < 0 ? 0 : lo - x0, b = hi - x0 > 31 ? 31 : hi - x0;
    return a > b ? 0u : bit_range((int)a, (int)b);
}

// the 32 bits sx .. sx + 31 of one row of `nw` words of array `array` (row_gather32 with every index checked)
__host__ __device__ inline uint32_t rule_gather(int array, const uint32_t* base, uint64_t row, uint64_t nw, int64_t sx)
{
    const int64_t k = sx >> 5;
    const int s = (int)(sx & 31);
    uint32_t lo = 0u, hi = 0u;
    if (k >= 0 && (uint64_t)k < nw) {
        VXRT_RULE_CHECK(array, row + (uint64_t)k);
        lo = base[row + (uint64_t)k];
    }
    if (s && k + 1 >= 0 && (uint64_t)(k + 1) < nw) {
        VXRT_RULE_CHECK(array, row + (uint64_t)(k + 1));
        hi = base[row + (uint64_t)(k + 1)];
    }
    (void)array;
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> s);
}

// a where m is set, b elsewhere (v_bfi)
__host__ __device__ inline uint32_t rule_select(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }

// ---- k_rule_setup: lane i = plane word ---------------------------------------------------------------------------------------
// the value lane i < kRuleSumWords gives summary word i before anything is tallied
__host__ __device__ inline uint32_t rule_summary_init(uint32_t i)
{
    return i >= kRuleSumMax ? (uint32_t)INT32_MIN : i >= kRuleSumMin ? (uint32_t)INT32_MAX : 0u;
}

// W_0's word completed (the voxels outside the world set when `outside` is 1) and F's word built
__host__ __device__ inline void rule_setup_lane(const RuleArgs& A, uint64_t i)
{
    const uint32_t xw = (uint32_t)(i % A.wh);
    const uint64_t row = i / A.wh;
    const uint32_t y = (uint32_t)(row % A.hy), z = (uint32_t)(row / A.hy);
    const int64_t h = A.h;
    const int64_t x0 = (int64_t)A.o[0] - h + 32 * (int64_t)xw, wy = (int64_t)A.o[1] - h + y, wz = (int64_t)A.o[2] - h + z;
    const uint32_t rmask = rule_span(32 * (int64_t)xw, 0, (int64_t)A.d[0] + 2 * h - 1);
    const bool yz_in = wy >= 0 && wy < A.dim[1] && wz >= 0 && wz < A.dim[2];
    const uint32_t in = yz_in ? rule_span(x0, 0, (int64_t)A.dim[0] - 1) & rmask : 0u;
    VXRT_RULE_CHECK(kRulePlane, i);
    if (A.outside)
        A.w0[i] |= rmask & ~in;
    uint32_t f = in;
    if (A.scope == kRuleBox) {
        const bool yz_box = y >= A.h && y < A.h + (uint32_t)A.d[1] && z >= A.h && z < A.h + (uint32_t)A.d[2];
        f = yz_box ? in & rule_span(32 * (int64_t)xw, h, h + A.d[0] - 1) : 0u;
        if (f && A.mask) {
            const uint64_t mrow = ((uint64_t)(y - A.h) + (uint64_t)A.d[1] * (z - A.h)) * A.mw;
            f &= rule_gather(kRuleMask, A.mask, mrow, A.mw, 32 * (int64_t)xw - h);
        }
    }
    A.free[i] = f;
}

// ---- k_rule_round: lane i = plane word -----------------------------------------------------------------------------------------
// what row (dy, dz) adds to the count in neighbourhood nb: 0 nothing, 1 its word, 2 the full row l + w + r, 3 (the centre
// row) l + r
constexpr int rule_row_kind(int nb, int dy, int dz)
{
    const int m = (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
    return m == 0 ? 3 : m == 1 ? (nb == kRuleN6 ? 1 : 2) : (nb == kRuleN6 ? 0 : nb == kRuleN18 ? 1 : 2);
}

// the two-bit number per voxel that the row of word w adds (p[0] the low plane); `in`: the row lies in the halo box
template <int KIND>
__host__ __device__ inline void rule_row(const RuleArgs& A, const uint32_t* src, uint64_t w, uint32_t xw, bool in, uint32_t p[2])
{
    p[0] = p[1] = 0u;
    if (KIND == 0 || !in)
        return;
    VXRT_RULE_CHECK(kRulePlane, w);
    const uint32_t c = src[w];
    if (KIND == 1) {
        p[0] = c;
        return;
    }
    uint32_t l = c << 1, r = c >> 1;  // bit j: the voxel at x - 1, at x + 1
    if (xw > 0u) {
        VXRT_RULE_CHECK(kRulePlane, w - 1u);
        l |= src[w - 1u] >> 31;
    }
    if (xw + 1u < A.wh) {
        VXRT_RULE_CHECK(kRulePlane, w + 1u);
        r |= src[w + 1u] << 31;
    }
    if (KIND == 2) {
        p[0] = l ^ c ^ r;
        p[1] = (l & c) | (r & (l ^ c));
    } else {
        p[0] = l ^ r;
        p[1] = l & r;
    }
}

template <int NB, int DY, int DZ>
__host__ __device__ inline void rule_row_at(const RuleArgs& A, const uint32_t* src, uint64_t i, uint32_t xw, uint32_t y, uint32_t z,
                                            uint32_t p[2])
{
    const bool in = (DY < 0 ? y > 0u : DY > 0 ? y + 1u < A.hy : true) && (DZ < 0 ? z > 0u : DZ > 0 ? z + 1u < A.hz : true);
    const int64_t w = (int64_t)i + DY * (int64_t)A.wh + DZ * (int64_t)A.wh * (int64_t)A.hy;
    rule_row<rule_row_kind(NB, DY, DZ)>(A, src, (uint64_t)w, xw, in, p);
}

// bit-sliced a + b: NA >= NB planes in, NA + 1 planes out
template <int NA, int NB>
__host__ __device__ inline void rule_add(const uint32_t* a, const uint32_t* b, uint32_t* out)
{
    uint32_t carry = 0u;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const uint32_t x = a[k], y = k < NB ? b[k] : 0u, t = x ^ y;
        out[k] = t ^ carry;
        carry = (x & y) | (carry & t);
    }
    out[NA] = carry;
}

// bit `count` of `table` per voxel, the count in five planes: a mux tree whose 32 leaves are the table's bits as all-ones
// or zero words
__host__ __device__ inline uint32_t rule_table(uint32_t table, const uint32_t c[5])
{
    uint32_t m[16];
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k)
        m[k] = rule_select(c[0], 0u - (table >> (2u * k + 1u) & 1u), 0u - (table >> (2u * k) & 1u));
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)
        m[k] = rule_select(c[1], m[2u * k + 1u], m[2u * k]);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        m[k] = rule_select(c[2], m[2u * k + 1u], m[2u * k]);
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k)
        m[k] = rule_select(c[3], m[2u * k + 1u], m[2u * k]);
    return rule_select(c[4], m[1], m[0]);
}

// the count of word i of `src` in five planes
template <int NB>
__host__ __device__ inline void rule_count(const RuleArgs& A, const uint32_t* src, uint64_t i, uint32_t cnt[6])
{
    const uint32_t xw = (uint32_t)(i % A.wh);
    const uint64_t row = i / A.wh;
    const uint32_t y = (uint32_t)(row % A.hy), z = (uint32_t)(row / A.hy);
    uint32_t a[2], b[2], t0[3], t1[3], u0[4], u1[4], v[5];
    rule_row_at<NB, -1, -1>(A, src, i, xw, y, z, a);
    rule_row_at<NB, 1, -1>(A, src, i, xw, y, z, b);
    rule_add<2, 2>(a, b, t0);
    rule_row_at<NB, -1, 1>(A, src, i, xw, y, z, a);
    rule_row_at<NB, 1, 1>(A, src, i, xw, y, z, b);
    rule_add<2, 2>(a, b, t1);
    rule_add<3, 3>(t0, t1, u0);  // the four corner rows
    rule_row_at<NB, 0, -1>(A, src, i, xw, y, z, a);
    rule_row_at<NB, 0, 1>(A, src, i, xw, y, z, b);
    rule_add<2, 2>(a, b, t0);
    rule_row_at<NB, -1, 0>(A, src, i, xw, y, z, a);
    rule_row_at<NB, 1, 0>(A, src, i, xw, y, z, b);
    rule_add<2, 2>(a, b, t1);
    rule_add<3, 3>(t0, t1, u1);  // the four edge rows
    rule_add<4, 4>(u0, u1, v);   // at most 24
    rule_row_at<NB, 0, 0>(A, src, i, xw, y, z, a);
    rule_add<5, 2>(v, a, cnt);   // at most 26: cnt[5] is 0
}

// word i of W_i+1 from the plane `src` that holds W_i
template <int NB>
__host__ __device__ inline uint32_t rule_round_word(const RuleArgs& A, const uint32_t* src, uint64_t i)
{
    uint32_t cnt[6];
    rule_count<NB>(A, src, i, cnt);
    VXRT_RULE_CHECK(kRulePlane, i);
    const uint32_t self = src[i];
    const uint32_t next = rule_select(self, rule_table(A.survive, cnt), rule_table(A.born, cnt));
    return rule_select(A.free[i], next, self);
}

template <int NB>
__host__ __device__ inline void rule_round_lane(const RuleArgs& A, const uint32_t* src, uint32_t* dst, uint64_t i)
{
    dst[i] = rule_round_word<NB>(A, src, i);
}

// ---- k_rule_output: lane i = word of d_bits, xb + mw * (y + dims[1] * z) ------------------------------------------------------------
// the tally of one lane, wave and workgroup: at most 2^28 voxels in all, so every count fits 32 bits
struct RuleTally {
    uint32_t n[5];  // solid_before, solid_after, born, died, changed_last
    int32_t lo[3], hi[3];
};

__host__ __device__ inline void rule_tally_clear(RuleTally& t)
{
    for (int k = 0; k < 5; ++k)
        t.n[k] = 0u;
    for (int k = 0; k < 3; ++k) {
        t.lo[k] = INT32_MAX;
        t.hi[k] = INT32_MIN;
    }
}

// `last`: the plane that holds W_n; `prev`: the plane that holds W_n-1
__host__ __device__ inline void rule_output_lane(const RuleArgs& A, const uint32_t* last, const uint32_t* prev, uint64_t i, RuleTally& t)
{
    const uint32_t xb = (uint32_t)(i % A.mw);
    const uint64_t row = i / A.mw;
    const uint32_t y = (uint32_t)(row % (uint32_t)A.d[1]), z = (uint32_t)(row / (uint32_t)A.d[1]);
    const int64_t x0 = (int64_t)A.o[0] + 32 * (int64_t)xb, wy = (int64_t)A.o[1] + y, wz = (int64_t)A.o[2] + z;
    // the world voxels of B in this word
    uint32_t m = 0u;
    if (wy >= 0 && wy < A.dim[1] && wz >= 0 && wz < A.dim[2])
        m = rule_span(x0, 0, (int64_t)A.dim[0] - 1) & rule_span(32 * (int64_t)xb, 0, (int64_t)A.d[0] - 1);
    const uint64_t hrow = (uint64_t)A.wh * ((uint64_t)(y + A.h) + (uint64_t)A.hy * (z + A.h));
    const int64_t sx = 32 * (int64_t)xb + A.h;
    const uint32_t wn = rule_gather(kRulePlane, last, hrow, A.wh, sx) & m;
    VXRT_RULE_CHECK(kRuleOut, i);
    A.out[i] = wn;
    if (!m)
        return;
    const uint32_t wp = rule_gather(kRulePlane, prev, hrow, A.wh, sx) & m;
    const uint32_t wz0 = rule_gather(kRulePlane, A.w0, hrow, A.wh, sx) & m;
    t.n[0] += (uint32_t)__builtin_popcount(wz0);
    t.n[1] += (uint32_t)__builtin_popcount(wn);
    t.n[2] += (uint32_t)__builtin_popcount(wn & ~wz0);
    t.n[3] += (uint32_t)__builtin_popcount(wz0 & ~wn);
    t.n[4] += (uint32_t)__builtin_popcount(wn ^ wp);
    const uint32_t ch = wn ^ wz0;
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

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_rule.hip on the box o, d
hipError_t apply_rule(const CollideWorld& W, const int32_t o[3], const int32_t d[3], const vxrt_rule& rule, const uint32_t* mask,
                      void* work, uint32_t* bits, vxrt_rule_summary* summary, hipStream_t stream);
#endif

}  // namespace vxrt
