// vxrt_lod.hpp -- occupancy LOD (include/vxrt.h, vxrt_downsample_region): the pieces shared by the kernels of
// vxrt_lod.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/lod_check.cpp, through
// tests/tools/hoststub): the limits and the workspace layout, the lane mapping, the bit-parallel count of a source word,
// the walk of one lane over the source rows of its cells and the counts, bits and tallies a lane ends with.
//
// Source.  The box S = dims << shift at `origin`, as k_read_region writes it: a row is wps = ceil(S[0] / 32) words, row
// (y, z) starts at word (y + S[1] * z) * wps, bits beyond S[0] and voxels outside the world are 0.
// Lane.  One lane owns one source word column k of one cell row (Y, Z): the n = 32 / f cells X = k * n + j, j < n, whose
// voxels along x are exactly the bits of word k.  It loads word k of the cell row's f * f source rows -- consecutive lanes
// load consecutive words -- and adds them in packed form:
//   field sums   `shift` SWAR stages turn a word into the sums of its f-bit fields (at most f each; at shift 5 the field is
//                the word and the sum is a popcount);
//   widening     for f <= 8 the even and the odd fields go to two accumulators with 2f-bit slots, which hold f^3 (8 in 4
//                bits, 64 in 8, 512 in 16); for f = 16 the two 16-bit fields hold 4096 as they are, for f = 32 the word holds
//                32768.
// Waves.  A wave task is 64 consecutive words of one cell row, or 64 / L cell rows of L <= 64 lanes each when a source row is
// shorter (L = wps rounded up to a power of two), as in k_read_region.  The f neighbouring lanes k = f * m .. f * m + f - 1
// hold the 32 bits of output word m (the L lanes of a row when L < f); an aligned group of lanes never straddles a wave.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_region.hpp"

// The harness defines this to check every index the code forms into the workspace or an output against that array's size
// (array: one of the kLod* ids below).  The kernels leave it empty.
#ifndef VXRT_LOD_CHECK
#define VXRT_LOD_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint32_t kLodMaxShift = 5;
constexpr uint64_t kLodMaxSource = 1ull << 32;  // voxels of the source box
enum { kLodSrc, kLodBits, kLodCounts, kLodArrays };

// the workspace (include/vxrt.h states the same formula) and the launch shape
struct LodLayout {
    uint64_t total_bytes;
    BoxFault fault;      // what lod_layout returned false for
    uint64_t nsrc;       // source words
    int32_t S[3];        // the source box
    uint32_t wps, wpo;   // words per source row, per output row
    uint32_t rows;       // cell rows: dims[1] * dims[2] (at most 2^29)
    uint32_t lgL, nxc;   // log2 of the lanes per cell row (L <= 64); 64-word chunks of a source row (1 when L < 64)
    uint32_t tasks;      // waves' worth of lanes: nxc * ceil(rows / (64 / L)), below 2^26
    uint32_t iters;      // tasks one wave takes in turn, so that a lane loads about 64 words: 16, 4, 1, 1, 1 by shift
};

// false outside the contract (L.fault: why): the shift, the dims and the source box and, when `o` is given, the origin
inline bool lod_layout(const int32_t* o, const int32_t d[3], uint32_t shift, LodLayout& L)
{
    L.fault = kBoxDims;
    if (shift < 1u || shift > kLodMaxShift)
        return false;
    uint64_t vox = 1u;
    for (int k = 0; k < 3; ++k) {
        if (d[k] < 1)
            return false;
        const uint64_t s = (uint64_t)d[k] << shift;  // < 2^36
        if (s > kLodMaxSource / vox)
            return false;
        vox *= s;  // <= 2^32
        L.S[k] = (int32_t)s;
    }
    L.fault = kBoxOrigin;
    for (int k = 0; k < 3; ++k)
        if (o && (int64_t)o[k] + L.S[k] > INT32_MAX)
            return false;
    L.fault = kBoxOk;
    L.nsrc = region_words(L.S);
    L.wps = (uint32_t)region_words_per_row(L.S[0]);
    L.wpo = (uint32_t)region_words_per_row(d[0]);
    L.rows = (uint32_t)d[1] * (uint32_t)d[2];
    L.lgL = 0;
    while ((1u << L.lgL) < L.wps && L.lgL < 6u)
        ++L.lgL;
    L.nxc = (L.wps + 63u) / 64u;
    const uint32_t rpw = 64u >> L.lgL;
    L.tasks = L.nxc * ((L.rows + rpw - 1u) / rpw);  // at most two lanes per source word of a cell row: 2 * 2^27 / 4 / 64
    L.iters = shift == 1u ? 16u : (shift == 2u ? 4u : 1u);
    L.total_bytes = section_up(4u * L.nsrc);
    return true;
}

// the threshold of a call: 1 .. f^3
inline bool lod_threshold_ok(uint32_t shift, uint32_t threshold)
{
    return shift >= 1u && shift <= kLodMaxShift && threshold >= 1u && threshold <= 1u << (3u * shift);
}

// what the reduce kernel reads and writes (device pointers; host pointers in the harness)
struct LodArgs {
    const uint32_t* src;  // the source box's region words (k_read_region)
    uint32_t* bits;       // output: region words of `dims`
    uint16_t* counts;     // output: one count per cell, or NULL
    void* summary;        // output: vxrt_lod_summary (zeroed before the launch)
    int32_t d[3];
    uint32_t shift, threshold;
    uint32_t s1;          // source rows per z slice: S[1]
    uint32_t wps, wpo, rows, lgL, nxc, iters;
};

inline void lod_args(LodArgs& A, const LodLayout& L, const int32_t d[3], uint32_t shift, uint32_t threshold, void* work,
                     uint32_t* bits, uint16_t* counts, void* summary)
{
    A.src = (const uint32_t*)work;
    A.bits = bits;
    A.counts = counts;
    A.summary = summary;
    for (int k = 0; k < 3; ++k)
        A.d[k] = d[k];
    A.shift = shift;
    A.threshold = threshold;
    A.s1 = (uint32_t)L.S[1];
    A.wps = L.wps;
    A.wpo = L.wpo;
    A.rows = L.rows;
    A.lgL = L.lgL;
    A.nxc = L.nxc;
    A.iters = L.iters;
}

// the tally of one lane over its cells
struct LodTally {
    uint32_t solid, set, empty, full, mixed, max_count;
};

// lane `lane` of wave task `task`: its source word column and its cell row; false when it has none
__host__ __device__ inline bool lod_lane(const LodArgs& A, uint32_t task, uint32_t lane, uint32_t& k, uint32_t& row)
{
    const uint32_t xc = task % A.nxc;
    const uint64_t r = (uint64_t)(task / A.nxc) * (64u >> A.lgL) + (lane >> A.lgL);
    k = xc * 64u + (lane & ((1u << A.lgL) - 1u));
    row = (uint32_t)r;
    return k < A.wps && r < A.rows;
}

// task i of the `iters` tasks that wave `wave` of the launch takes in turn: consecutive tasks, so consecutive rows
__host__ __device__ inline uint32_t lod_wave_task(uint32_t wave, uint32_t iters, uint32_t i) { return wave * iters + i; }

// the sums of the f-bit fields of a word, f = 1 << SH, each in its field
template <uint32_t SH>
__host__ __device__ inline uint32_t lod_field_sums(uint32_t x)
{
    if (SH == 5u)
        return (uint32_t)__builtin_popcount(x);
    x = x - ((x >> 1) & 0x55555555u);  // 2-bit fields: 0 .. 2
    if (SH >= 2u)
        x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);  // 4-bit fields: 0 .. 4
    if (SH >= 3u)
        x = (x + (x >> 4)) & 0x0F0F0F0Fu;  // 8-bit fields: 0 .. 8 (the sum of two fields still fits one)
    if (SH >= 4u)
        x = (x + (x >> 8)) & 0x00FF00FFu;  // 16-bit fields: 0 .. 16
    return x;
}

// Word k of the source rows of cell row (Y, Z) in the slices dz0 <= dz < dz1 of the cell, added to the accumulators: `lo`
// takes the even fields and `hi` the odd ones in 2f-bit slots (f <= 8); for f >= 16 `lo` takes the sums as they are.
template <uint32_t SH>
__host__ __device__ inline void lod_accumulate(const LodArgs& A, uint32_t k, uint32_t Y, uint32_t Z, uint32_t dz0, uint32_t dz1,
                                               uint32_t& lo, uint32_t& hi)
{
    constexpr uint32_t f = 1u << SH;
    constexpr uint32_t even = SH == 1u ? 0x33333333u : (SH == 2u ? 0x0F0F0F0Fu : 0x00FF00FFu);
    for (uint32_t dz = dz0; dz < dz1; ++dz) {
        uint64_t i = ((uint64_t)Y * f + (uint64_t)A.s1 * ((uint64_t)Z * f + dz)) * A.wps + k;
        for (uint32_t dy = 0; dy < f; ++dy, i += A.wps) {
            VXRT_LOD_CHECK(kLodSrc, i);
            const uint32_t x = lod_field_sums<SH>(A.src[i]);
            if (SH <= 3u) {
                lo += x & even;
                hi += (x >> f) & even;
            } else {
                lo += x;
            }
        }
    }
}

// the count of cell j of the lane's word from its accumulators
template <uint32_t SH>
__host__ __device__ inline uint32_t lod_count(uint32_t lo, uint32_t hi, uint32_t j)
{
    constexpr uint32_t f = 1u << SH;
    if (SH == 5u)
        return lo;
    if (SH == 4u)
        return (lo >> (16u * j)) & 0xFFFFu;
    return (((j & 1u) ? hi : lo) >> (f * (j & ~1u))) & ((1u << (2u * f)) - 1u);
}

// The lane's cells: their counts written (when asked for), tallied, and compared with the threshold.  Returns the cells'
// bits where they lie in the output word k >> SH; cells at or beyond dims[0] produce nothing.
template <uint32_t SH>
__host__ __device__ inline uint32_t lod_finish(const LodArgs& A, uint32_t k, uint32_t row, uint32_t lo, uint32_t hi, LodTally& t)
{
    constexpr uint32_t f = 1u << SH, n = 32u >> SH, full = f * f * f;
    const uint32_t X0 = k * n;
    const uint64_t base = (uint64_t)row * (uint32_t)A.d[0] + X0;
    uint32_t bits = 0u;
    for (uint32_t j = 0; j < n && X0 + j < (uint32_t)A.d[0]; ++j) {
        const uint32_t c = lod_count<SH>(lo, hi, j);
        if (A.counts) {
            VXRT_LOD_CHECK(kLodCounts, base + j);
            A.counts[base + j] = (uint16_t)c;
        }
        t.solid += c;
        t.empty += c == 0u;
        t.full += c == full;
        t.mixed += c != 0u && c != full;
        t.max_count = c > t.max_count ? c : t.max_count;
        if (c >= A.threshold) {
            ++t.set;
            bits |= 1u << j;
        }
    }
    return bits << ((k & (f - 1u)) * n);
}

// the lanes that hold one output word: f, or the L lanes of a cell row when a source row is shorter than f words
__host__ __device__ inline uint32_t lod_group(const LodArgs& A)
{
    const uint32_t f = 1u << A.shift, L = 1u << A.lgL;
    return f < L ? f : L;
}

// the word of a group's first lane goes to the output: `word` is the OR of the group's lanes
__host__ __device__ inline void lod_store(const LodArgs& A, uint32_t k, uint32_t row, uint32_t word)
{
    if (k & ((1u << A.shift) - 1u))
        return;
    const uint64_t i = (uint64_t)row * A.wpo + (k >> A.shift);
    VXRT_LOD_CHECK(kLodBits, i);
    A.bits[i] = word;
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_lod.hip on the box o, d
hipError_t downsample_region(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t shift, uint32_t threshold,
                             void* work, uint32_t* bits, uint16_t* counts, vxrt_lod_summary* summary, hipStream_t stream);
#endif

}  // namespace vxrt
