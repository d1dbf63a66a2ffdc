// vxrt_light.hpp -- voxel light fields (include/vxrt.h, vxrt_light_field): the pieces shared by the kernels of
// vxrt_light.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/light_check.cpp, through
// tests/tools/hoststub): the workspace layout and, one lane at a time, the work of every launch.
//
// Halo.  H = 14.  Halo voxel (hx, hy, hz) is world voxel origin - H + (hx, hy, hz), so voxel (x, y, z) of B is halo voxel
// (x + H, y + H, z + H).  A PLANE is one bit per halo voxel in vxrt_read_region's layout: wh = ceil(h[0] / 32) words per
// row, word xw + wh * (hy + h[1] * hz).  The halo's solid bits come from k_read_region (outside the world: 0) and are
// inverted in place into the EMPTY plane, a row's padding bits kept 0: nothing dilates through them.
// Level sets.  S_k = the voxels of level >= k.  S_15 = sources of level 15 (sky: the exposed voxels; block: the emitters of
// level 15), S_k = (dilate6(S_k+1) | sources of level k) & empty for k = 14 .. 1, two planes per channel in turn.  dilate6 of
// a word: itself, itself shifted one bit each way with the carry bit of the neighbouring word of the row, and the words of
// the four neighbouring rows; a neighbour outside the halo box adds nothing.
// Level.  The sets are nested, so level(v) = how many of S_1 .. S_15 hold v.  Four LEVEL planes per channel keep the count
// of S_15 .. S_2 bit-sliced: the round that reads S_k+1 adds it with a ripple (t = L[b] & c; L[b] ^= c; c = t) that stops at
// the first zero carry; S_1 is added when the planes are read out.
// Emitters.  One record per entry (plane word, bit, level; 0 when the entry is not used).  After the round that stored S_k
// the used emitters of level k are ORed into it: OR only, so the order of the entries and of the lanes changes nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into an array of the workspace, the emitters or the output
// against that array's size (array: one of the kLight* ids below).  The kernels leave it empty.
#ifndef VXRT_LIGHT_CHECK
#define VXRT_LIGHT_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint64_t kLightMaxVoxels = 1ull << 28;
constexpr uint32_t kLightMax = 15, kLightHalo = 14, kLightMaxEmitters = 65536;
constexpr uint32_t kLightSky = 1, kLightBlock = 2;
constexpr uint32_t kLightSlab = 8;   // rows of the columns above the halo one lane ORs together
enum { kLightPlane, kLightAbove, kLightRec, kLightEmit, kLightOut, kLightSummary };
// summary words (vxrt_light_summary); the sums are the uint64 at words 34, 35 and 36, 37
enum {
    kLightSumSolid = 0, kLightSumExposed = 1, kLightSumHist = 2, kLightSumSum = 34, kLightSumUsed = 38, kLightSumWords = 42
};

// the workspace: sections of bytes, each on a 256-byte boundary (include/vxrt.h states the same formula).  Channel slot 0
// is the sky channel when it is requested, else the block channel.
struct LightLayout : HaloBox {  // the halo box (vxrt_region.hpp): B grown by H
    uint64_t empty, above, set[2][2], level[2], rec;  // byte offsets (set[slot][turn], level[slot]: four planes)
    uint64_t total_bytes;
    uint64_t np, nabove;  // words of a plane (= nhalo), of the blocked-above mask
    uint32_t nvox, nch;   // voxels of B, channels requested
};

// false outside the contract (L.fault: why): channels, dims, the halo box within a region read and, when `o` is given,
// within int32
inline bool light_layout(const int32_t* o, const int32_t d[3], uint32_t channels, LightLayout& L)
{
    L.fault = channels < 1 || channels > 3 ? kBoxDims : halo_box(o, d, (int32_t)kLightHalo, kLightMaxVoxels, L);
    if (L.fault != kBoxOk)
        return false;
    L.np = L.nhalo;
    L.nvox = (uint32_t)box_voxels(d, kLightMaxVoxels);
    L.nabove = (uint64_t)L.wh * L.hz;
    L.nch = (channels & kLightSky ? 1u : 0u) + (channels & kLightBlock ? 1u : 0u);
    Sections S;  // (a section that is not requested takes nothing and shares the next one's offset)
    L.empty = S.take(4u * L.np);
    L.above = S.take((channels & kLightSky) ? 4u * L.nabove : 0u);
    for (uint32_t c = 0; c < 2; ++c) {
        const uint64_t plane = c < L.nch ? section_up(4u * L.np) : 0u;
        L.set[c][0] = S.take(plane);
        L.set[c][1] = S.take(plane);
        L.level[c] = S.take(4u * plane);
    }
    L.rec = S.take((channels & kLightBlock) ? 8u * (uint64_t)kLightMaxEmitters : 0u);
    L.total_bytes = S.at;
    return true;
}

// what the light kernels read and write (device pointers; host pointers in the harness)
struct LightArgs {
    uint32_t* empty;         // the halo's solid bits, then (k_light_columns) its empty bits
    uint32_t* above;         // xw + wh * hz: some solid voxel in the column above the halo
    uint32_t* set[2][2];     // [slot][turn]: the level sets, two planes in turn
    uint32_t* level[2];      // [slot]: four planes, plane b at + b * np
    uint64_t* rec;           // one record per emitter: word << 9 | bit << 4 | level, 0 when not used
    const int32_t* emitters; // n_emitters x (x, y, z, level)
    uint8_t* out;            // output: d_levels
    uint32_t* summary;       // output: vxrt_light_summary
    uint64_t np;
    int32_t o[3], d[3];
    uint32_t channels, nch, sky, block;  // sky, block: the channel's slot, 2 when it is not requested
    uint32_t n_emitters;
    uint32_t wh, hy, hz;
    uint32_t wide;           // the output may be stored four bytes at a time (its address is a multiple of 4)
};

inline void light_args(LightArgs& A, const LightLayout& L, const int32_t o[3], const int32_t d[3], uint32_t channels, void* work,
                       const int32_t* emitters, uint32_t n_emitters, uint8_t* out, uint32_t* summary)
{
    char* w = (char*)work;
    A.empty = (uint32_t*)(w + L.empty);
    A.above = (uint32_t*)(w + L.above);
    for (int c = 0; c < 2; ++c) {
        A.set[c][0] = (uint32_t*)(w + L.set[c][0]);
        A.set[c][1] = (uint32_t*)(w + L.set[c][1]);
        A.level[c] = (uint32_t*)(w + L.level[c]);
    }
    A.rec = (uint64_t*)(w + L.rec);
    A.emitters = emitters;
    A.out = out;
    A.summary = summary;
    A.np = L.np;
    for (int k = 0; k < 3; ++k) {
        A.o[k] = o[k];
        A.d[k] = d[k];
    }
    A.channels = channels;
    A.nch = L.nch;
    A.sky = (channels & kLightSky) ? 0u : 2u;
    A.block = (channels & kLightBlock) ? L.nch - 1u : 2u;
    A.n_emitters = (channels & kLightBlock) ? n_emitters : 0u;
    A.wh = L.wh;
    A.hy = L.hy;
    A.hz = L.hz;
    A.wide = ((uintptr_t)out & 3u) == 0u ? 1u : 0u;
}

// the bits of word xw of a halo row that are voxels of the halo (the rest is padding)
__host__ __device__ inline uint32_t light_row_mask(const LightArgs& A, uint32_t xw)
{
    const uint32_t rem = ((uint32_t)A.d[0] + 2u * kLightHalo) & 31u;
    return (xw == A.wh - 1u && rem) ? (1u << rem) - 1u : 0xFFFFFFFFu;
}

// the bits of word xw of a halo row that are voxels of B along x: halo voxels H .. H + dims[0] - 1
__host__ __device__ inline uint32_t light_box_mask(const LightArgs& A, uint32_t xw)
{
    const int64_t lo = (int64_t)kLightHalo - 32 * (int64_t)xw, hi = lo + A.d[0] - 1;  // the range in this word's bits
    if (hi < 0 || lo > 31)
        return 0u;
    return bit_range(lo < 0 ? 0 : (int)lo, hi > 31 ? 31 : (int)hi);
}

// ---- k_light_above: lane i = xw + wh * (hz + h[2] * slab) ---------------------------------------------------------------
// the first world row above the halo, and how many slabs of kLightSlab rows reach from it to the world's top
inline int64_t light_above_first(const LightArgs& A)
{
    const int64_t top = (int64_t)A.o[1] + A.d[1] + kLightHalo;
    return top < 0 ? 0 : top;
}
inline uint32_t light_above_slabs(const LightArgs& A, const CollideWorld& W)
{
    const int64_t rows = (int64_t)W.dim[1] - light_above_first(A);
    return rows > 0 ? (uint32_t)((rows + kLightSlab - 1) / kLightSlab) : 0u;
}

// the solid bits of up to kLightSlab world rows of one (xw, hz) column above the halo, ORed into the mask.  Clipped to the
// world before any load, as k_read_region clips.
__host__ __device__ inline void light_above_lane(const LightArgs& A, const CollideWorld& W, int64_t first, uint64_t i)
{
    const uint32_t xw = (uint32_t)(i % A.wh);
    const uint64_t q = i / A.wh;
    const uint32_t hz = (uint32_t)(q % A.hz), slab = (uint32_t)(q / A.hz);
    const int64_t x0 = (int64_t)A.o[0] - kLightHalo + 32 * (int64_t)xw, wz = (int64_t)A.o[2] - kLightHalo + hz;
    if (wz < 0 || wz >= W.dim[2] || x0 + 31 < 0 || x0 >= W.dim[0])
        return;
    const int64_t y0 = first + (int64_t)slab * kLightSlab;
    uint32_t any = 0u;
    for (int64_t y = y0; y < y0 + kLightSlab && y < W.dim[1]; ++y)
        any |= region_row_word(W.meta, W.pool, W.f, W.lgf, W.cx, W.cz, x0, (int)y, (int)wz);
    any &= light_row_mask(A, xw);
    if (any) {
        VXRT_LIGHT_CHECK(kLightAbove, xw + (uint64_t)A.wh * hz);
        atom_or(A.above + xw + (uint64_t)A.wh * hz, any);
    }
}

// ---- k_light_columns: lane i = xw + wh * hz, down the halo's rows --------------------------------------------------------
// The column's words turned from solid to empty bits in place and, with the sky channel, its exposed bits stored as S_15:
// exposed(y) = exposed(y + 1) & empty(y), from ~blocked above.  Returns the exposed voxels of B in the column.
__host__ __device__ inline uint32_t light_column_lane(const LightArgs& A, uint64_t i)
{
    const uint32_t xw = (uint32_t)(i % A.wh), hz = (uint32_t)(i / A.wh);
    const uint32_t rmask = light_row_mask(A, xw);
    const bool sky = A.sky < 2u;
    uint32_t exposed = 0u, count = 0u;
    if (sky) {
        VXRT_LIGHT_CHECK(kLightAbove, i);
        exposed = ~A.above[i] & rmask;
    }
    const bool z_in = hz >= kLightHalo && hz < kLightHalo + (uint32_t)A.d[2];
    const uint32_t bmask = z_in ? light_box_mask(A, xw) : 0u;
    const uint64_t base = (uint64_t)xw + (uint64_t)A.wh * (uint64_t)A.hy * hz;
    // from the top row down, eight rows at a time: the eight loads are in flight together, then the dependent pass
    for (uint32_t top = A.hy; top > 0u;) {
        const uint32_t n = top < 8u ? top : 8u;
        uint32_t e[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            if (k < n) {
                const uint64_t w = base + (uint64_t)A.wh * (top - 1u - k);
                VXRT_LIGHT_CHECK(kLightPlane, w);
                e[k] = ~A.empty[w] & rmask;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            if (k < n) {
                const uint32_t y = top - 1u - k;
                const uint64_t w = base + (uint64_t)A.wh * y;
                A.empty[w] = e[k];
                if (sky) {
                    exposed &= e[k];
                    A.set[A.sky][0][w] = exposed;
                    if (y >= kLightHalo && y < kLightHalo + (uint32_t)A.d[1])
                        count += (uint32_t)__builtin_popcount(exposed & bmask);
                }
            }
        }
        top -= n;
    }
    return count;
}

// ---- k_light_classify: lane e, one emitter -----------------------------------------------------------------------------------
// the entry's class (0 used, 1 solid, 2 far, 3 invalid: the order of the summary's counts) and its record
__host__ __device__ inline uint32_t light_classify_lane(const LightArgs& A, uint32_t e)
{
    VXRT_LIGHT_CHECK(kLightEmit, 4u * (uint64_t)e + 3u);
    VXRT_LIGHT_CHECK(kLightRec, e);
    const int32_t* p = A.emitters + 4u * (uint64_t)e;
    const int32_t level = p[3];
    A.rec[e] = 0u;
    if (level < 1 || level > (int32_t)kLightMax)
        return 3u;
    int64_t h[3];
    for (int k = 0; k < 3; ++k) {
        h[k] = (int64_t)p[k] - ((int64_t)A.o[k] - kLightHalo);
        if (h[k] < 0 || h[k] >= (int64_t)A.d[k] + 2 * (int64_t)kLightHalo)
            return 2u;
    }
    const uint64_t w = (uint64_t)(h[0] >> 5) + (uint64_t)A.wh * ((uint64_t)h[1] + (uint64_t)A.hy * (uint64_t)h[2]);
    const uint32_t bit = (uint32_t)h[0] & 31u;
    VXRT_LIGHT_CHECK(kLightPlane, w);
    if (!((A.empty[w] >> bit) & 1u))
        return 1u;
    A.rec[e] = w << 9 | (uint64_t)bit << 4 | (uint64_t)level;
    return 0u;
}

// ---- k_light_scatter: lane e, the used emitters of level k ORed into `plane` -----------------------------------------------------
__host__ __device__ inline void light_scatter_lane(const LightArgs& A, uint32_t* plane, uint32_t k, uint32_t e)
{
    VXRT_LIGHT_CHECK(kLightRec, e);
    const uint64_t r = A.rec[e];
    if ((uint32_t)(r & 15u) != k)
        return;
    VXRT_LIGHT_CHECK(kLightPlane, r >> 9);
    atom_or(plane + (r >> 9), 1u << ((uint32_t)(r >> 4) & 31u));
}

// ---- k_light_round: lane i = plane word + np * slot ------------------------------------------------------------------------------
// Round `turn` (0 .. 13) reads S_k+1 = set[slot][turn & 1] with k = 14 - turn, adds it to the level planes and stores
// S_k = dilate6(S_k+1) & empty into set[slot][~turn & 1].
__host__ __device__ inline void light_round_lane(const LightArgs& A, uint32_t turn, uint64_t i)
{
    const uint32_t c = (uint32_t)(i / A.np);
    const uint64_t w = i % A.np;
    const uint32_t* src = A.set[c][turn & 1u];
    uint32_t* dst = A.set[c][~turn & 1u];
    uint32_t* lev = A.level[c];
    const uint32_t xw = (uint32_t)(w % A.wh);
    const uint64_t row = w / A.wh;
    const uint32_t y = (uint32_t)(row % A.hy), z = (uint32_t)(row / A.hy);
    const uint64_t sy = A.wh, sz = (uint64_t)A.wh * A.hy;
    VXRT_LIGHT_CHECK(kLightPlane, w);
    const uint32_t s = src[w];
    // the count of the sets so far, bit-sliced: plane b += carry
    uint32_t carry = s;
    for (uint32_t b = 0; b < 4u; ++b) {
        if (turn == 0u) {
            lev[b * A.np + w] = b ? 0u : s;
        } else if (carry) {
            const uint32_t t = lev[b * A.np + w];
            lev[b * A.np + w] = t ^ carry;
            carry &= t;
        }
    }
    uint32_t g = s | s << 1 | s >> 1;
    if (xw > 0u) {
        VXRT_LIGHT_CHECK(kLightPlane, w - 1u);
        g |= src[w - 1u] >> 31;
    }
    if (xw + 1u < A.wh) {
        VXRT_LIGHT_CHECK(kLightPlane, w + 1u);
        g |= src[w + 1u] << 31;
    }
    if (y > 0u) {
        VXRT_LIGHT_CHECK(kLightPlane, w - sy);
        g |= src[w - sy];
    }
    if (y + 1u < A.hy) {
        VXRT_LIGHT_CHECK(kLightPlane, w + sy);
        g |= src[w + sy];
    }
    if (z > 0u) {
        VXRT_LIGHT_CHECK(kLightPlane, w - sz);
        g |= src[w - sz];
    }
    if (z + 1u < A.hz) {
        VXRT_LIGHT_CHECK(kLightPlane, w + sz);
        g |= src[w + sz];
    }
    dst[w] = g & A.empty[w];
}

// the level bits of plane word w of a slot as four planes: the count of S_15 .. S_2 plus S_1 (set[slot][0] after round 13);
// at most 15, so the last carry is always 0
__host__ __device__ inline void light_level_planes(const LightArgs& A, uint32_t c, uint64_t w, uint32_t p[4])
{
    VXRT_LIGHT_CHECK(kLightPlane, w);
    const uint32_t* last = c ? A.set[1][0] : A.set[0][0];  // selects, not an index into the arguments
    const uint32_t* lev = c ? A.level[1] : A.level[0];
    uint32_t carry = last[w];
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t t = lev[b * A.np + w];
        p[b] = t ^ carry;
        carry &= t;
    }
}

// ---- k_light_expand: lane j, the bytes 4 j .. 4 j + 3 of the output -------------------------------------------------------------
__host__ __device__ inline void light_expand_lane(const LightArgs& A, uint64_t j)
{
    const uint64_t nvox = (uint64_t)A.d[0] * (uint64_t)A.d[1] * (uint64_t)A.d[2];
    const uint64_t v0 = 4u * j;
    const uint32_t n = nvox - v0 < 4u ? (uint32_t)(nvox - v0) : 4u;
    uint32_t x = (uint32_t)(v0 % (uint32_t)A.d[0]);
    uint64_t row = v0 / (uint32_t)A.d[0];  // y + dims[1] * z
    uint32_t sky[4] = {0u, 0u, 0u, 0u}, blk[4] = {0u, 0u, 0u, 0u}, packed = 0u;
    uint64_t have = ~0ull;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t y = (uint32_t)(row % (uint32_t)A.d[1]), z = (uint32_t)(row / (uint32_t)A.d[1]);
        const uint32_t hx = x + kLightHalo, bit = hx & 31u;
        const uint64_t w = (uint64_t)(hx >> 5) + (uint64_t)A.wh * ((uint64_t)(y + kLightHalo) + (uint64_t)A.hy * (z + kLightHalo));
        if (w != have) {
            have = w;
            if (A.sky < 2u)
                light_level_planes(A, A.sky, w, sky);
            if (A.block < 2u)
                light_level_planes(A, A.block, w, blk);
        }
        uint32_t v = 0u;
        for (uint32_t b = 0; b < 4u; ++b)
            v |= ((sky[b] >> bit) & 1u) << (4u + b) | ((blk[b] >> bit) & 1u) << b;
        packed |= v << (8u * k);
        if (++x == (uint32_t)A.d[0]) {
            x = 0u;
            ++row;
        }
    }
    VXRT_LIGHT_CHECK(kLightOut, v0 + n - 1u);
    if (n == 4u && A.wide) {
        *(uint32_t*)(A.out + v0) = packed;
    } else {
        for (uint32_t k = 0; k < n; ++k)
            A.out[v0 + k] = (uint8_t)(packed >> (8u * k));
    }
}

// ---- k_light_tally: lane i = xi + nxb * (y + dims[1] * z), one halo word that holds voxels of B -----------------------------------
// the tally of one lane, wave and workgroup over one channel (ch 0 sky, 1 block; the solid voxels are counted with channel
// 0): at most 2^28 voxels in all, so every count fits 32 bits.  One channel at a time keeps 17 counters in registers.
struct LightTally {
    uint32_t solid;
    uint32_t hist[16];
};

// halo words per row that hold voxels of B: words 0 .. (H + dims[0] - 1) / 32
__host__ __device__ inline uint32_t light_box_words(const LightArgs& A) { return ((kLightHalo + (uint32_t)A.d[0] - 1u) >> 5) + 1u; }

__host__ __device__ inline void light_tally_lane(const LightArgs& A, uint32_t ch, uint64_t i, LightTally& t)
{
    const uint32_t nxb = light_box_words(A);
    const uint32_t xw = (uint32_t)(i % nxb);
    const uint64_t row = i / nxb;
    const uint32_t y = (uint32_t)(row % (uint32_t)A.d[1]), z = (uint32_t)(row / (uint32_t)A.d[1]);
    const uint64_t w = (uint64_t)xw + (uint64_t)A.wh * ((uint64_t)(y + kLightHalo) + (uint64_t)A.hy * (z + kLightHalo));
    const uint32_t bmask = light_box_mask(A, xw);
    VXRT_LIGHT_CHECK(kLightPlane, w);
    const uint32_t e = A.empty[w] & bmask;
    if (ch == 0u)
        t.solid += (uint32_t)__builtin_popcount(~A.empty[w] & bmask);
    const uint32_t slot = ch ? A.block : A.sky;
    uint32_t p[4] = {0u, 0u, 0u, 0u};  // a channel that is not requested: level 0 everywhere
    if (slot < 2u)
        light_level_planes(A, slot, w, p);
#pragma unroll
    for (uint32_t l = 0; l < 16u; ++l) {
        uint32_t m = e;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b)
            m &= (l >> b & 1u) ? p[b] : ~p[b];
        t.hist[l] += (uint32_t)__builtin_popcount(m);
    }
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_light.hip on the box o, d
hipError_t light_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t channels, const int32_t* emitters,
                       uint32_t n_emitters, void* work, uint8_t* levels, vxrt_light_summary* summary, hipStream_t stream);
#endif

}  // namespace vxrt
