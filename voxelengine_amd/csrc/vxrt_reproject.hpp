// vxrt_reproject.hpp -- the temporal filter (include/vxrt.h, vxrt_reproject_frame): the per-pixel logic shared by the kernel
// of vxrt_reproject.hip, the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/
// reproject_check.cpp, through tests/tools/hoststub): the limits, the hit point of a pixel on its face plane, its position
// in the previous camera's frame, the four taps with their weights, the blend and the stores.
//
// The frame and the shared helpers are vxrt_frame.hpp's; the launch shape of every frame stage is defined here ("launch").  The history is one 16-byte record {r, g, b, n} per
// pixel: a tap is one dwordx4 load and one key load.  A pixel reads its own colour and key and the four taps of the previous
// frame, and writes its own record, colour and BGRA8 pixel.
#pragma once

#include "vxrt_frame.hpp"

// The harness defines this to check every index the code forms into an input or an output against that array's size
// (array: one of the kRp* ids below).  The kernel leaves it empty.
#ifndef VXRT_RP_CHECK
#define VXRT_RP_CHECK(array, index)
#endif

namespace vxrt {

constexpr int32_t kRpMaxHistory = 65535;
enum { kRpColorIn, kRpKeys, kRpHistIn, kRpKeysPrev, kRpHistOut, kRpColorOut, kRpFb, kRpArrays };
// what became of a pixel (the counters of vxrt_reproject_summary: a hit pixel is one of the last three)
enum { kRpMiss, kRpReused, kRpOffscreen, kRpRejected };

inline bool reproject_history_ok(int32_t max_history) { return max_history >= 1 && max_history <= kRpMaxHistory; }

struct alignas(16) RpRec {
    float r, g, b, n;
};

// what the launch reads and writes (device pointers; host pointers in the harness)
struct ReprojectArgs {
    const float* color_in;      // W * H * 3
    const uint32_t* keys;       // W * H
    const RpRec* hist_in;       // W * H, or NULL together with keys_prev: no history
    const uint32_t* keys_prev;  // W * H
    RpRec* hist_out;            // W * H
    float* color_out;           // W * H * 3, or NULL
    uint32_t* fb;               // W * H BGRA8 pixels, or NULL
    uint32_t* summary;          // hit, reused, offscreen, rejected, or NULL
    uint32_t W, H;
    int32_t ortho;
    float max_history;
    float kx, ky, ortho_x, ortho_y, ratio;  // the constants of camera_args
    float po[3], pf[3], pu[3], pr[3];       // the previous camera: origin, fwd, up, right
};

// Where the surface point that pixel of key `key` and primary ray (o, d) shows lay in the previous frame: (fx, fy) in pixel
// units; false when it has no such position (the contract's steps 2 and 3).
__host__ __device__ inline bool rp_previous_position(const ReprojectArgs& A, uint32_t key, const float o[3], const float d[3], float& fx,
                                                     float& fy)
{
    const FrameFace face = frame_face(key);
    const uint32_t a = face.a;  // (the clamp of frame_face changes none of the selects below)
    const float pl = face.pl;
    float da;
    const float t = frame_plane_t(a, pl, o, d, da);
    if (da == 0.0f || !frame_finite(t))
        return false;
    const float P[3] = {a == 0u ? pl : o[0] + t * d[0], a == 1u ? pl : o[1] + t * d[1], a >= 2u ? pl : o[2] + t * d[2]};
    const float r[3] = {P[0] - A.po[0], P[1] - A.po[1], P[2] - A.po[2]};
    float su, sv;
    if (A.ortho) {
        su = frame_dot(r, A.pr) / (A.ortho_x * A.ratio);
        sv = frame_dot(r, A.pu) / A.ortho_y;
    } else {
        const float z = frame_dot(r, A.pf);
        if (!(z > 0.0f))
            return false;
        su = frame_dot(r, A.pr) / (z * A.kx);
        sv = frame_dot(r, A.pu) / (z * A.ky);
    }
    fx = ((su + 1.0f) * 0.5f) * (float)A.W;
    fy = ((sv + 1.0f) * 0.5f) * (float)A.H;
    return fx >= -1.0f && fx <= (float)A.W && fy >= -1.0f && fy <= (float)A.H;  // (a NaN fails)
}

// Pixel (x, y) with primary ray (o, d): its record, colour and BGRA8 pixel stored; returns what became of it (kRp*).
// The four history taps and the four key taps are loaded unconditionally, from the pixel's own index where a tap has no
// address of its own, so that the eight loads of a lane are in flight together; what a tap that is not accepted holds is
// never used -- a select, not an addition of zero, so that a NaN behind a foreign key stays out.
__host__ __device__ inline uint32_t rp_pixel(const ReprojectArgs& A, uint32_t x, uint32_t y, const float o[3], const float d[3])
{
    const uint32_t i = y * A.W + x;  // W * H <= 2^26: every index fits 32 bits
    VXRT_RP_CHECK(kRpColorIn, 3u * i + 2u);
    VXRT_RP_CHECK(kRpKeys, i);
    const float c[3] = {A.color_in[3u * i], A.color_in[3u * i + 1u], A.color_in[3u * i + 2u]};
    const uint32_t key = A.keys[i];
    float fx = 0.0f, fy = 0.0f;
    const bool onscreen = key != 0u && rp_previous_position(A, key, o, d, fx, fy);
    fx = onscreen ? fx : 0.0f;
    fy = onscreen ? fy : 0.0f;
    const float flx = floorf(fx), fly = floorf(fy);
    const float wx = fx - flx, wy = fy - fly;
    const int32_t x0 = (int32_t)flx, y0 = (int32_t)fly;  // -1 .. 65535 (0 when not onscreen)
    const float w[4] = {(1.0f - wx) * (1.0f - wy), wx * (1.0f - wy), (1.0f - wx) * wy, wx * wy};
    bool inside[4];
    uint32_t at[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t qx = x0 + (j & 1), qy = y0 + (j >> 1);
        inside[j] = onscreen && qx >= 0 && qy >= 0 && qx < (int32_t)A.W && qy < (int32_t)A.H;
        at[j] = inside[j] ? (uint32_t)qy * A.W + (uint32_t)qx : i;
    }
    RpRec h[4];
    uint32_t kq[4];
    const bool history = A.hist_in != nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (history) {
            VXRT_RP_CHECK(kRpHistIn, at[j]);
            VXRT_RP_CHECK(kRpKeysPrev, at[j]);
            h[j] = A.hist_in[at[j]];
            kq[j] = A.keys_prev[at[j]];
        } else {
            h[j] = RpRec{0.0f, 0.0f, 0.0f, 0.0f};
            kq[j] = 0u;
        }
    }
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, nmin = __builtin_huge_valf();
    bool any_inside = false, any_used = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool use = inside[j] && w[j] > 0.0f && kq[j] == key && h[j].n >= 1.0f;
        any_inside = any_inside || inside[j];
        any_used = any_used || use;
        sw = use ? sw + w[j] : sw;
        sr = use ? sr + w[j] * h[j].r : sr;
        sg = use ? sg + w[j] * h[j].g : sg;
        sb = use ? sb + w[j] * h[j].b : sb;
        nmin = use && h[j].n < nmin ? h[j].n : nmin;
    }
    RpRec out{c[0], c[1], c[2], key != 0u ? 1.0f : 0.0f};
    if (any_used) {
        const float mr = sr / sw, mg = sg / sw, mb = sb / sw;
        const float n1 = nmin + 1.0f, n = n1 < A.max_history ? n1 : A.max_history;
        out = RpRec{mr + (c[0] - mr) / n, mg + (c[1] - mg) / n, mb + (c[2] - mb) / n, n};
    }
    VXRT_RP_CHECK(kRpHistOut, i);
    A.hist_out[i] = out;
    if (A.color_out) {
        VXRT_RP_CHECK(kRpColorOut, 3u * i + 2u);
        const float rgb[3] = {out.r, out.g, out.b};
        frame_store_color(A.color_out, i, rgb);
    }
    if (A.fb) {
        VXRT_RP_CHECK(kRpFb, i);
        A.fb[i] = dn_bgra8(out.r, out.g, out.b);
    }
    return key == 0u ? kRpMiss : any_used ? kRpReused : any_inside ? kRpRejected : kRpOffscreen;
}

// ---- launch ------------------------------------------------------------------------------------------------------------
// A tile is 64 x 4 pixels: four waves, wave j of them on row j, lanes along x.  Wave `gw` of the launch (workgroup * waves
// per workgroup + wave in it) belongs to the group of four gw / 4 and has row gw % 4 of that group's tiles; the group takes the
// tiles group, group + groups, ... of the ceil(W / 64) * ceil(H / 4) tiles, row-major.
// Without a summary a workgroup is one group of four waves on one tile (kRpPlain): the most waves in flight.  With a summary
// the counters of a wave's tiles stay in its registers, the waves of a workgroup add theirs in LDS and one lane issues the
// workgroup's atomics, so the launch is few large workgroups (kRpCounted lanes, `cus * kRpCountedPerCu` of them at most), each
// wave on several tiles: every atomicAdd of a launch hits the same 16 bytes and they serialise there, at about 12 ns each
// (profiles/reproject.md: one set per wave of a 1080p frame cost 0.8 ms beside a 45 us kernel).
constexpr uint32_t kRpPlain = 256u, kRpCounted = 1024u, kRpCountedPerCu = 2u;

// the lanes of a workgroup: the one rule that the launch, the kernel body (frame_stage) and the harnesses take them from
constexpr uint32_t rp_block(bool summary) { return summary ? kRpCounted : kRpPlain; }

inline uint32_t rp_tiles(uint32_t W, uint32_t H) { return ((W + 63u) / 64u) * ((H + 3u) / 4u); }  // <= 1024 * 16384

inline void rp_launch_shape(uint32_t W, uint32_t H, bool summary, uint32_t cus, uint32_t& block, uint32_t& grid)
{
    const uint32_t tiles = rp_tiles(W, H);
    block = rp_block(summary);
    grid = tiles;
    if (summary) {
        const uint32_t most = (cus ? cus : 1u) * kRpCountedPerCu, need = (tiles + kRpCounted / 256u - 1u) / (kRpCounted / 256u);
        grid = need < most ? need : most;
    }
}

// wave `gw` of a launch of `waves` waves: the pixel of its lane `lane` in its i-th tile; false past the wave's last tile
__host__ __device__ inline bool rp_wave_pixel(uint32_t W, uint32_t H, uint32_t gw, uint32_t waves, uint32_t i, uint32_t lane, uint32_t& x,
                                              uint32_t& y)
{
    const uint32_t gx = (W + 63u) / 64u, tiles = gx * ((H + 3u) / 4u);
    const uint64_t t = (uint64_t)(gw >> 2) + (uint64_t)i * (waves >> 2);
    if (t >= tiles)
        return false;
    x = (uint32_t)(t % gx) * 64u + lane;
    y = (uint32_t)(t / gx) * 4u + (gw & 3u);
    return true;
}

#ifndef VXRT_HOST_CHECK  // the kernel of vxrt_reproject.hip
struct RenderArgs;  // (vxrt_kernels.hpp)
// R carries the current camera (camera_args, ortho, origin, fwd, up, right), A the rest; cus: the device's compute units
hipError_t reproject_frame(const RenderArgs& R, const ReprojectArgs& A, uint32_t cus, hipStream_t stream);
#endif

}  // namespace vxrt
