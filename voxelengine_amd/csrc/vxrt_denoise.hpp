// vxrt_denoise.hpp -- the edge-avoiding frame denoiser (include/vxrt.h, vxrt_frame_guides / vxrt_denoise_frame): the pieces
// shared by the kernels of vxrt_denoise.hip, the host side in vxrt_api_query.hip and the host harness of the tests
// (tests/tools/denoise_check.cpp, through tests/tools/hoststub): the limits and the workspace formula, the guide key of a
// pixel from its hit index and primary ray, the record of the ping-pong workspace, the tile a workgroup owns, the staging
// of a tile with its halo, the 25 taps of a pixel in the order the contract fixes, and the stores.
//
// Frame.  W x H pixels, x fastest.  The workspace is two buffers of one 16-byte record {r, g, b, key bits} per pixel; a tap
// is one dwordx4 load.  Iteration i reads buffer (i - 1) & 1 and writes buffer i & 1; iteration 0 reads the float3 input and
// the keys instead (the pack is fused), the last one writes the float3 output and the BGRA8 pixel instead (the unpack is
// fused), so a call with one iteration touches no workspace at all.
// Tile.  A workgroup of 256 lanes owns 64 x (4 * ROWS) pixels: wave w has the rows w, w + 4, ..., lanes along x, so every
// tap row of a wave is 64 consecutive records (1 KB).  DIRECT (ROWS = 1) reads its taps from memory; STAGED (ROWS = 4)
// first copies the tile and its halo of 2 * step pixels into LDS -- positions outside the frame as key 0, which equals no
// filtered pixel's key -- and reads its taps there (step <= kDnMaxStagedStep: beyond that the halo outgrows the tile).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// The harness defines this to check every index the code forms into an input, the workspace, an output or the LDS tile
// against that array's size (array: one of the kDn* ids below).  The kernels leave it empty.
#ifndef VXRT_DN_CHECK
#define VXRT_DN_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint32_t kDnMaxSide = 65535u;
constexpr uint64_t kDnMaxPixels = 1ull << 26;
constexpr int32_t kDnMaxIterations = 6;
constexpr uint32_t kDnMaxAxis = 1u << 24;  // world voxels per axis: a face plane is an integer a binary32 holds, below 2^25
constexpr uint32_t kDnMaxStagedStep = 2u;
constexpr uint32_t kDnTileW = 64u, kDnStagedRows = 4u;
// the staged tile with its halo at the largest staged step
constexpr uint32_t kDnLdsRecords = (kDnTileW + 4u * kDnMaxStagedStep) * (4u * kDnStagedRows + 4u * kDnMaxStagedStep);
enum { kDnColorIn, kDnKeys, kDnSrc, kDnDst, kDnColorOut, kDnFb, kDnLds, kDnArrays };

inline bool denoise_frame_ok(uint32_t W, uint32_t H)
{
    return W >= 1u && H >= 1u && W <= kDnMaxSide && H <= kDnMaxSide && (uint64_t)W * H <= kDnMaxPixels;
}

// the workspace (include/vxrt.h states the same formula)
inline uint64_t denoise_workspace_bytes(uint32_t W, uint32_t H) { return denoise_frame_ok(W, H) ? 2ull * W * H * 16ull : 0ull; }

// ---- guide keys --------------------------------------------------------------------------------------------------------
// The face of voxel `hit`'s box that the ray (o, d) enters: 1<<31 | axis<<26 | toward<<25 | plane; 0 for a miss (-1) or an
// index outside the X * Y * Z voxels.  X, Y, Z <= kDnMaxAxis.
__host__ __device__ inline uint32_t guide_key(long long hit, uint32_t X, uint32_t Y, uint32_t Z, const float o[3], const float d[3])
{
    if (hit < 0)
        return 0u;
    const uint64_t xy = (uint64_t)X * Y, z = (uint64_t)hit / xy, r = (uint64_t)hit % xy;
    if (z >= Z)
        return 0u;
    const uint32_t v[3] = {(uint32_t)(r % X), (uint32_t)(r / X), (uint32_t)z};
    uint32_t axis = 0u, plane = 0u;
    float best = 0.0f;
    for (uint32_t k = 0; k < 3u; ++k) {
        const uint32_t p = d[k] > 0.0f ? v[k] : v[k] + 1u;
        const float t = d[k] != 0.0f ? ((float)p - o[k]) / d[k] : -__builtin_huge_valf();
        if (k == 0u || t > best) {
            best = t;
            axis = k;
            plane = p;
        }
    }
    return 0x80000000u | (axis << 26) | ((d[axis] > 0.0f ? 1u : 0u) << 25) | plane;
}

// ---- filter ------------------------------------------------------------------------------------------------------------
struct alignas(16) DnRec {
    float r, g, b;
    uint32_t key;
};

// what one iteration reads and writes (device pointers; host pointers in the harness)
struct DenoiseArgs {
    const float* color_in;   // first iteration: W * H * 3
    const uint32_t* keys;    // first iteration: W * H
    const DnRec* src;        // later iterations
    DnRec* dst;              // all but the last iteration
    float* color_out;        // last iteration: W * H * 3
    uint32_t* fb;            // last iteration: W * H BGRA8 pixels, or NULL
    uint32_t W, H, step;
    float k;                 // colour stop, >= 0; 0 = none
    int32_t last;
};

// the pixel (x, y) of the frame as the iteration reads it (FIRST: from the float3 colours and the keys); W * H <= 2^26, so
// every index fits 32 bits
template <bool FIRST>
__host__ __device__ inline DnRec dn_load(const DenoiseArgs& A, uint32_t x, uint32_t y)
{
    const uint32_t i = y * A.W + x;
    if (FIRST) {
        VXRT_DN_CHECK(kDnColorIn, 3u * i + 2u);
        VXRT_DN_CHECK(kDnKeys, i);
        return DnRec{A.color_in[3u * i], A.color_in[3u * i + 1u], A.color_in[3u * i + 2u], A.keys[i]};
    }
    VXRT_DN_CHECK(kDnSrc, i);
    return A.src[i];
}

// setPixelColor's rule (Renderer.cu:72-87, PixelSink::put of vxrt_kernels.hip): clamp, *255, truncate; bytes b, g, r, 255
__host__ __device__ inline uint32_t dn_bgra8(float r, float g, float b)
{
    r = r > 0.0f ? r : 0.0f;
    g = g > 0.0f ? g : 0.0f;
    b = b > 0.0f ? b : 0.0f;
    r = r < 1.0f ? r : 1.0f;
    g = g < 1.0f ? g : 1.0f;
    b = b < 1.0f ? b : 1.0f;
    return (uint32_t)(b * 255) | ((uint32_t)(g * 255) << 8) | ((uint32_t)(r * 255) << 16) | 0xFF000000u;
}

__host__ __device__ inline void dn_store(const DenoiseArgs& A, uint32_t x, uint32_t y, const DnRec& c)
{
    const uint32_t i = y * A.W + x;
    if (!A.last) {
        VXRT_DN_CHECK(kDnDst, i);
        A.dst[i] = c;
        return;
    }
    VXRT_DN_CHECK(kDnColorOut, 3u * i + 2u);
    A.color_out[3u * i] = c.r;
    A.color_out[3u * i + 1u] = c.g;
    A.color_out[3u * i + 2u] = c.b;
    if (A.fb) {
        VXRT_DN_CHECK(kDnFb, i);
        A.fb[i] = dn_bgra8(c.r, c.g, c.b);
    }
}

// The filtered pixel p from its taps, in the contract's order: dy outer, dx inner, binary32, no contraction.
// tap(dx, dy, q): the record at p + step * (dx, dy) into q, false when that lies outside the frame (q is then some record of
// the frame: the load is unconditional, so that the 25 loads of a lane are in flight together).  A skipped tap leaves the
// sums as they are -- a select, not an addition of zero, so that a NaN or an infinity behind a foreign key stays out.
template <class Tap>
__host__ __device__ inline DnRec dn_filter(const DnRec& p, float k, Tap&& tap)
{
    if (p.key == 0u)
        return p;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            DnRec q;
            const bool inside = tap(dx, dy, q), use = inside && q.key == p.key;
            const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
            const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
            const float er = q.r - p.r, eg = q.g - p.g, eb = q.b - p.b;
            const float d2 = (er * er + eg * eg) + eb * eb;
            const float stop = 1.0f - d2 * k;
            const float w = k > 0.0f ? (hx * hy) * (stop > 0.0f ? stop : 0.0f) : hx * hy;  // (selects: one basic block)
            sw = use ? sw + w : sw;
            sr = use ? sr + w * q.r : sr;
            sg = use ? sg + w * q.g : sg;
            sb = use ? sb + w * q.b : sb;
        }
    }
    return DnRec{sr / sw, sg / sw, sb / sw, p.key};
}

// the LDS tile of a STAGED workgroup: (kDnTileW + 4 step) x (4 ROWS + 4 step) records, row-major
__host__ __device__ inline uint32_t dn_tile_width(uint32_t step) { return kDnTileW + 4u * step; }
__host__ __device__ inline uint32_t dn_tile_height(uint32_t step) { return 4u * kDnStagedRows + 4u * step; }

// lane `tid` of workgroup (bx, by) copies its share of the tile and its halo into `tile`
template <bool FIRST>
__host__ __device__ inline void dn_stage(const DenoiseArgs& A, uint32_t bx, uint32_t by, uint32_t tid, DnRec* tile)
{
    const uint32_t tw = dn_tile_width(A.step), n = tw * dn_tile_height(A.step);
    const int32_t halo = 2 * (int32_t)A.step;
    const int32_t x0 = (int32_t)(bx * kDnTileW) - halo, y0 = (int32_t)(by * (4u * kDnStagedRows)) - halo;
    for (uint32_t i = tid; i < n; i += 256u) {
        const int32_t x = x0 + (int32_t)(i % tw), y = y0 + (int32_t)(i / tw);
        DnRec q{0.0f, 0.0f, 0.0f, 0u};
        if (x >= 0 && y >= 0 && x < (int32_t)A.W && y < (int32_t)A.H)
            q = dn_load<FIRST>(A, (uint32_t)x, (uint32_t)y);
        VXRT_DN_CHECK(kDnLds, i);
        tile[i] = q;
    }
}

// lane `tid` of workgroup (bx, by) filters and stores its pixels: one (DIRECT) or kDnStagedRows (STAGED, after dn_stage
// of every lane of the workgroup)
template <bool STAGED, bool FIRST>
__host__ __device__ inline void dn_compute(const DenoiseArgs& A, uint32_t bx, uint32_t by, uint32_t tid, const DnRec* tile)
{
    constexpr uint32_t rows = STAGED ? kDnStagedRows : 1u;
    const uint32_t lane = tid & 63u, wave = tid >> 6, x = bx * kDnTileW + lane;
    const int32_t s = (int32_t)A.step;
    if (x >= A.W)
        return;
    for (uint32_t j = 0; j < rows; ++j) {
        const uint32_t ly = wave + 4u * j, y = by * (4u * rows) + ly;
        if (y >= A.H)
            return;
        DnRec c;
        if (STAGED) {
            const uint32_t tw = dn_tile_width(A.step), centre = (ly + 2u * A.step) * tw + lane + 2u * A.step;
            VXRT_DN_CHECK(kDnLds, centre);
            c = dn_filter(tile[centre], A.k, [&](int dx, int dy, DnRec& q) {
                const uint32_t i = (uint32_t)((int32_t)centre + s * (dy * (int32_t)tw + dx));
                VXRT_DN_CHECK(kDnLds, i);
                q = tile[i];
                return true;  // outside the frame: key 0, equal to no filtered pixel's
            });
        } else {
            c = dn_filter(dn_load<FIRST>(A, x, y), A.k, [&](int dx, int dy, DnRec& q) {
                const int32_t qx = (int32_t)x + s * dx, qy = (int32_t)y + s * dy;  // |s * d| <= 64 beside at most 65534
                const bool inside = qx >= 0 && qy >= 0 && qx < (int32_t)A.W && qy < (int32_t)A.H;
                q = dn_load<FIRST>(A, inside ? (uint32_t)qx : x, inside ? (uint32_t)qy : y);
                return inside;
            });
        }
        dn_store(A, x, y, c);
    }
}

// the launch grid of one iteration
inline void dn_grid(uint32_t W, uint32_t H, bool staged, uint32_t& gx, uint32_t& gy)
{
    const uint32_t th = 4u * (staged ? kDnStagedRows : 1u);
    gx = (W + kDnTileW - 1u) / kDnTileW;
    gy = (H + th - 1u) / th;
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_denoise.hip
struct RenderArgs;  // (vxrt_kernels.hpp)
hipError_t frame_guides(const RenderArgs& R, uint32_t Z, uint32_t* keys, hipStream_t stream);
hipError_t denoise_frame(uint32_t W, uint32_t H, const float* color_in, const uint32_t* keys, int32_t iterations, float k,
                         void* work, float* color_out, void* fb, hipStream_t stream);
#endif

}  // namespace vxrt
