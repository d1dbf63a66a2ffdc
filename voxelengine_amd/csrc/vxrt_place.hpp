// vxrt_place.hpp -- voxel piece queries (include/vxrt.h, vxrt_place_pieces): the pieces shared by the kernels of
// vxrt_place.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/place_check.cpp, through
// tests/tools/hoststub): placement validation, the launch shape, the overlap count of one piece row at one offset, the
// 32-step x window of one piece row, and the three per-lane passes (init, sweep, contact) and the finish.
//
// A task is (placement, chunk of `lanes` piece rows); lane l of the task owns row chunk * lanes + l of the piece (rows run y
// fastest, then z, as in the region layout).  The results are the accumulators: word 1 of a result holds the first blocked
// step (|dist| + 1 while none is known) until place_finish turns it into the travel.  Everything is integer arithmetic, and
// the tasks of a placement combine through a minimum and two sums, so no result depends on the order the tasks run in.
// Every world row is gathered with region_row_word (vxrt_region.hpp) after its y and z were tested against the world.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxrt_device.hpp"
#include "vxrt_region.hpp"

// The harness defines these to check every index the code forms: VXRT_PLACE_CHECK(array, index) for the placements, the
// results and a piece's words (array kPlaceWords + piece), VXRT_PLACE_CHECK_ROW for a world row before its gather.
#ifndef VXRT_PLACE_CHECK
#define VXRT_PLACE_CHECK(array, index)
#endif
#ifndef VXRT_PLACE_CHECK_ROW
#define VXRT_PLACE_CHECK_ROW(W, x0, y, z)
#endif

namespace vxrt {

constexpr uint32_t kPlaceMaxPieces = 64;       // VXRT_PLACE_MAX_PIECES
constexpr int32_t kPlaceMaxDim = 1024;         // VXRT_PLACE_MAX_DIM
constexpr uint64_t kPlaceMaxVoxels = 1u << 24; // VXRT_PLACE_MAX_VOXELS
constexpr int32_t kPlaceMaxDist = 4096;        // VXRT_PLACE_MAX_DIST
constexpr int32_t kPlaceMaxCoord = 1 << 30;    // |origin[k]| <= 2^30
constexpr uint32_t kPlacedBlocked = 1u, kPlacedInvalid = 2u;
constexpr uint32_t kPlaceNone = 0xFFFFFFFFu;
enum { kPlacePlacements = 0, kPlaceResults = 1, kPlaceWords = 2 };  // array ids of VXRT_PLACE_CHECK (kPlaceWords + piece)

struct PlacePiece {
    const uint32_t* bits;  // device, region layout
    int32_t d[3];
    uint32_t wpr;  // words per row
};

// one call as the kernels read it; the piece descriptors travel by value
struct PlaceArgs {
    CollideWorld W;
    const int32_t* placements;  // n x 6: piece, origin[3], axis, dist
    uint32_t* results;          // n x 4: overlap, first blocked step -> travel, contact, flags
    uint64_t n;
    uint32_t n_pieces;
    uint32_t lanes;  // lanes (rows) of a task: a power of two, 1 .. 64
    uint32_t tasks;  // tasks of a placement: ceil(most rows of a piece / lanes)
    uint32_t pad_;
    PlacePiece pieces[kPlaceMaxPieces];
};

// 0 = a piece within the contract: dims 1 .. 1024 each, at most 2^24 voxels, bits not NULL, reserved 0
inline int piece_prepare(const uint32_t* bits, const int32_t d[3], int32_t reserved, PlacePiece& out)
{
    if (!bits || reserved != 0)
        return -1;
    for (int k = 0; k < 3; ++k)
        if (d[k] < 1 || d[k] > kPlaceMaxDim)
            return -1;
    if ((uint64_t)d[0] * (uint64_t)d[1] * (uint64_t)d[2] > kPlaceMaxVoxels)
        return -1;
    out.bits = bits;
    for (int k = 0; k < 3; ++k)
        out.d[k] = d[k];
    out.wpr = (uint32_t)region_words_per_row(d[0]);
    return 0;
}

// the launch shape of a batch: as many lanes per task as the piece with the most rows fills (a power of two up to 64), and
// as many tasks per placement as that piece needs; a piece with fewer rows leaves its surplus tasks empty
inline void place_shape(PlaceArgs& A)
{
    uint32_t rows = 1;
    for (uint32_t k = 0; k < A.n_pieces; ++k) {
        const uint32_t r = (uint32_t)A.pieces[k].d[1] * (uint32_t)A.pieces[k].d[2];
        rows = r > rows ? r : rows;
    }
    uint32_t lanes = 1;
    while (lanes < 64 && lanes < rows)
        lanes <<= 1;
    A.lanes = lanes;
    A.tasks = (rows + lanes - 1) / lanes;
}

// ---- the lanes of a task as one: a reduction over the `lanes` lanes that share a task (aligned groups of a wave).  The host
// harness runs one lane at a time, every lane its own group: minima and sums then meet in the results' atomics instead. ----
#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline uint32_t group_sum(uint32_t v, uint32_t lanes)
{
    for (uint32_t m = lanes >> 1; m; m >>= 1)
        v += (uint32_t)__shfl_xor((int)v, (int)m, 64);
    return v;
}
__device__ inline uint32_t group_min(uint32_t v, uint32_t lanes)
{
    for (uint32_t m = lanes >> 1; m; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, (int)m, 64);
        v = o < v ? o : v;
    }
    return v;
}
// the value of the group's first lane
__device__ inline uint32_t group_first(uint32_t v, uint32_t lanes)
{
    return (uint32_t)__shfl((int)v, (int)((threadIdx.x & 63u) & ~(lanes - 1u)), 64);
}
__device__ inline bool group_leader(uint32_t lane) { return lane == 0u; }
#else
inline uint32_t group_sum(uint32_t v, uint32_t) { return v; }
inline uint32_t group_min(uint32_t v, uint32_t) { return v; }
inline uint32_t group_first(uint32_t v, uint32_t) { return v; }
inline bool group_leader(uint32_t) { return true; }
#endif

// the placement rule of include/vxrt.h
__host__ __device__ inline bool place_valid(const int32_t p[6], uint32_t n_pieces)
{
    if (p[0] < 0 || (uint32_t)p[0] >= n_pieces || p[4] < 0 || p[4] > 2)
        return false;
    if (p[5] < -kPlaceMaxDist || p[5] > kPlaceMaxDist)
        return false;
    for (int k = 1; k <= 3; ++k)
        if (p[k] < -kPlaceMaxCoord || p[k] > kPlaceMaxCoord)
            return false;
    return true;
}

// the mask of the voxels of word w of a piece row (the padding bits of the last word are not voxels)
__host__ __device__ __forceinline__ uint32_t piece_word_mask(const PlacePiece& P, uint32_t w)
{
    return w + 1u == P.wpr ? bit_range(0, (P.d[0] - 1) & 31) : 0xFFFFFFFFu;
}

__host__ __device__ __forceinline__ uint32_t piece_word(const PlacePiece& P, int piece, uint64_t row, uint32_t w)
{
    VXRT_PLACE_CHECK(kPlaceWords + piece, row * P.wpr + w);
    return P.bits[row * P.wpr + w] & piece_word_mask(P, w);
}

__host__ __device__ __forceinline__ uint32_t place_world_word(const CollideWorld& W, int64_t x0, int y, int z)
{
    if (x0 + 31 < 0 || x0 >= W.dim[0])
        return 0u;
    VXRT_PLACE_CHECK_ROW(W, x0, y, z);
    return region_row_word(W.meta, W.pool, W.f, W.lgf, W.cx, W.cz, x0, y, z);
}

// one lane's row of a placement: where it lies in the world with the piece at its origin
struct PlaceRow {
    uint64_t row;  // row of the piece
    int64_t x;     // world x of the row's bit 0
    int y, z;      // world row
    uint32_t w0;   // the row's first word, masked: a row of up to 32 voxels is not loaded again at every step
    bool any;      // the row holds a voxel
};

// word w of the row's piece bits, masked
__host__ __device__ __forceinline__ uint32_t place_row_word(const PlacePiece& P, int piece, const PlaceRow& R, uint32_t w)
{
    return w == 0u ? R.w0 : piece_word(P, piece, R.row, w);
}

// the solid world voxels the row's voxels meet with the piece displaced by `off` along `axis`; zero piece words are skipped
// before any world load, a row outside the world in y or z meets nothing
__host__ __device__ __forceinline__ uint32_t place_row_count(const CollideWorld& W, const PlacePiece& P, int piece, const PlaceRow& R,
                                                    int axis, int off)
{
    const int y = R.y + (axis == 1 ? off : 0), z = R.z + (axis == 2 ? off : 0);
    if (y < 0 || y >= W.dim[1] || z < 0 || z >= W.dim[2])
        return 0u;
    const int64_t x = R.x + (axis == 0 ? off : 0);
    uint32_t count = 0u;
    for (uint32_t w = 0; w < P.wpr; ++w) {
        const uint32_t pw = place_row_word(P, piece, R, w);
        if (pw)
            count += (uint32_t)__builtin_popcount(pw & place_world_word(W, x + 32 * (int64_t)w, y, z));
    }
    return count;
}

// the least step j of [j0 + 1, min(j0 + 32, lim)] along x in direction s at which the row meets a solid voxel, or kPlaceNone.
// One 64-bit window of world bits per piece word answers the 32 steps: step j0 + 1 + t reads the window shifted by t (s > 0:
// the window starts at x + j0 + 1) or by 31 - t (s < 0: the window starts at x - j0 - 32).
__host__ __device__ __forceinline__ uint32_t place_row_first_x(const CollideWorld& W, const PlacePiece& P, int piece, const PlaceRow& R, int s,
                                                      uint32_t j0, uint32_t lim)
{
    if (R.y < 0 || R.y >= W.dim[1] || R.z < 0 || R.z >= W.dim[2])
        return kPlaceNone;
    uint32_t nt = lim - j0 > 32u ? 32u : lim - j0;  // steps still open in this window
    uint32_t best = kPlaceNone;
    for (uint32_t w = 0; w < P.wpr && nt; ++w) {
        const uint32_t pw = place_row_word(P, piece, R, w);
        if (!pw)
            continue;
        const int64_t x0 = R.x + 32 * (int64_t)w + (s > 0 ? (int64_t)j0 + 1 : -(int64_t)j0 - 32);
        const uint64_t v = (uint64_t)place_world_word(W, x0, R.y, R.z) | (uint64_t)place_world_word(W, x0 + 32, R.y, R.z) << 32;
        if (!v)
            continue;
        for (uint32_t t = 0; t < nt; ++t)
            if (pw & (uint32_t)(v >> (s > 0 ? t : 31u - t))) {
                best = j0 + 1u + t;
                nt = t;  // later words can only improve on it
                break;
            }
    }
    return best;
}

// the row of lane `lane` of task `chunk` of a placement p of piece P; false: the lane has no row
__host__ __device__ __forceinline__ bool place_row(const PlacePiece& P, int piece, const int32_t p[6], uint64_t row, PlaceRow& R)
{
    R.any = false;
    R.w0 = 0u;
    if (row >= (uint64_t)P.d[1] * (uint64_t)P.d[2])
        return false;
    const int py = (int)(row % (uint32_t)P.d[1]), pz = (int)(row / (uint32_t)P.d[1]);
    R.row = row;
    R.x = p[1];
    R.y = p[2] + py;
    R.z = p[3] + pz;
    R.w0 = piece_word(P, piece, row, 0u);
    uint32_t any = R.w0;
    for (uint32_t w = 1; w < P.wpr; ++w)
        any |= piece_word(P, piece, row, w);
    R.any = any != 0u;
    return true;
}

__host__ __device__ __forceinline__ void place_load(const PlaceArgs& A, uint64_t i, int32_t p[6])
{
    for (int k = 0; k < 6; ++k) {
        VXRT_PLACE_CHECK(kPlacePlacements, i * 6 + k);
        p[k] = A.placements[i * 6 + k];
    }
}

// ---- pass 0, one lane per placement: {0, |dist| + 1, 0, 0}, or {0, 0, 0, INVALID} --------------------------------------
__host__ __device__ inline void place_init(const PlaceArgs& A, uint64_t i)
{
    int32_t p[6];
    place_load(A, i, p);
    const bool ok = place_valid(p, A.n_pieces);
    const uint32_t ad = (uint32_t)(p[5] < 0 ? -p[5] : p[5]);
    const uint32_t r[4] = {0u, ok ? ad + 1u : 0u, 0u, ok ? 0u : kPlacedInvalid};
    for (int k = 0; k < 4; ++k) {
        VXRT_PLACE_CHECK(kPlaceResults, i * 4 + k);
        A.results[i * 4 + k] = r[k];
    }
}

// ---- pass 1, lane `lane` of task `task`: the row's overlap at the origin added to word 0, and the sweep.  Steps are tested
// nearest first by the lanes of the task together; the task stops at the first step at which one of its rows is blocked, and
// at once where another task of the placement already found a nearer one (word 1, read before every step). ----------------
__host__ __device__ inline void place_sweep(const PlaceArgs& A, uint64_t task, uint32_t lane)
{
    const uint64_t i = task / A.tasks;
    const uint32_t chunk = (uint32_t)(task % A.tasks);
    int32_t p[6];
    place_load(A, i, p);
    if (!place_valid(p, A.n_pieces))
        return;
    const PlacePiece& P = A.pieces[p[0]];
    if ((uint64_t)chunk * A.lanes >= (uint64_t)P.d[1] * (uint64_t)P.d[2])
        return;  // the whole task lies behind the piece's last row
    PlaceRow R;
    place_row(P, p[0], p, (uint64_t)chunk * A.lanes + lane, R);
    const int axis = p[4];

    const uint32_t ov = group_sum(R.any ? place_row_count(A.W, P, p[0], R, axis, 0) : 0u, A.lanes);
    if (ov && group_leader(lane)) {
        VXRT_PLACE_CHECK(kPlaceResults, i * 4);
        atom_add(&A.results[i * 4], ov);
    }

    const uint32_t ad = (uint32_t)(p[5] < 0 ? -p[5] : p[5]);
    if (ad == 0u)
        return;
    const int s = p[5] < 0 ? -1 : 1;
    VXRT_PLACE_CHECK(kPlaceResults, i * 4 + 1);
    uint32_t* first = &A.results[i * 4 + 1];
    uint32_t lim = ad;  // steps 1 .. lim are still open
    for (uint32_t j = 0; j < lim;) {  // steps 1 .. j are free in this task's rows
        if (A.tasks > 1u) {
            const uint32_t seen = group_first(atom_load(first), A.lanes) - 1u;  // first >= 1
            lim = seen < lim ? seen : lim;
            if (j >= lim)
                break;
        }
        uint32_t hit;
        if (axis == 0) {
            hit = group_min(R.any ? place_row_first_x(A.W, P, p[0], R, s, j, lim) : kPlaceNone, A.lanes);
            j += 32u;
        } else {
            ++j;
            const bool here = R.any && place_row_count(A.W, P, p[0], R, axis, s * (int)j) != 0u;
            hit = group_min(here ? j : kPlaceNone, A.lanes);
        }
        if (hit != kPlaceNone) {
            if (group_leader(lane))
                atom_min(first, hit);
            break;
        }
    }
}

// ---- pass 2, the lanes of pass 1 again: a blocked placement's contact, ov(first blocked step), added to word 2 -----------
__host__ __device__ inline void place_contact(const PlaceArgs& A, uint64_t task, uint32_t lane)
{
    const uint64_t i = task / A.tasks;
    const uint32_t chunk = (uint32_t)(task % A.tasks);
    int32_t p[6];
    place_load(A, i, p);
    if (!place_valid(p, A.n_pieces))
        return;
    const uint32_t ad = (uint32_t)(p[5] < 0 ? -p[5] : p[5]);
    VXRT_PLACE_CHECK(kPlaceResults, i * 4 + 1);
    const uint32_t first = A.results[i * 4 + 1];
    if (first > ad)
        return;
    const PlacePiece& P = A.pieces[p[0]];
    if ((uint64_t)chunk * A.lanes >= (uint64_t)P.d[1] * (uint64_t)P.d[2])
        return;
    PlaceRow R;
    place_row(P, p[0], p, (uint64_t)chunk * A.lanes + lane, R);
    const int off = p[5] < 0 ? -(int)first : (int)first;
    const uint32_t c = group_sum(R.any ? place_row_count(A.W, P, p[0], R, p[4], off) : 0u, A.lanes);
    if (c && group_leader(lane)) {
        VXRT_PLACE_CHECK(kPlaceResults, i * 4 + 2);
        atom_add(&A.results[i * 4 + 2], c);
    }
}

// ---- pass 3, one lane per placement: the first blocked step becomes the signed travel and the BLOCKED flag ---------------
__host__ __device__ inline void place_finish(const PlaceArgs& A, uint64_t i)
{
    int32_t p[6];
    place_load(A, i, p);
    if (!place_valid(p, A.n_pieces))
        return;
    const uint32_t ad = (uint32_t)(p[5] < 0 ? -p[5] : p[5]);
    VXRT_PLACE_CHECK(kPlaceResults, i * 4 + 3);
    const uint32_t first = A.results[i * 4 + 1];
    const int32_t k = (int32_t)first - 1;
    A.results[i * 4 + 1] = (uint32_t)(p[5] < 0 ? -k : k);
    A.results[i * 4 + 3] = first <= ad ? kPlacedBlocked : 0u;
}

#ifndef VXRT_HOST_CHECK
hipError_t place_pieces(const PlaceArgs& A, hipStream_t stream);  // the kernels of vxrt_place.hip
#endif

}  // namespace vxrt
