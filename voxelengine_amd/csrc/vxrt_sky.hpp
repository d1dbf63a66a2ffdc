// vxrt_sky.hpp -- sky on frames (include/vxrt.h, vxrt_sky_frame): the per-pixel logic shared by the kernel of vxrt_sky.hip,
// the host side in vxrt_api_query.hip and the host harnesses of the tests (tests/tools/sky_check.cpp and sky_args_check.cpp,
// through tests/tools/hoststub): the checks of the parameters, the sky without disc and clouds (sky_base), the cloud noise
// (sky_value, sky_vnoise, sky_clouds), the miss pixel, the fog of a hit pixel and the stores.
//
// The frame and the shared helpers are vxrt_frame.hpp's, the launch is the temporal filter's (rp_launch_shape,
// rp_wave_pixel).  A pixel reads its own key and, on a hit, its own colour, and writes its own colour and BGRA8 pixel.  Nothing here calls libm but floorf: the host and the device forms give
// the same bits.
#pragma once

#include "vxrt_reproject.hpp"  // the launch shape (and with it vxrt_frame.hpp)

// The harness defines this to check every index the code forms into an input or an output against that array's size
// (array: one of the kSky* ids below).  The kernel leaves it empty.
#ifndef VXRT_SKY_CHECK
#define VXRT_SKY_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint32_t kSkyClouds = 1u;  // VXRT_SKY_CLOUDS
constexpr uint32_t kSkyMaxGlowLog2 = 8u, kSkyMaxOctaves = 6u, kSkyCounters = 6u;
enum { kSkyColorIn, kSkyKeys, kSkyColorOut, kSkyFb, kSkyArrays };
// what became of a pixel: the counters of vxrt_sky_summary it adds to, bit k for counter k
enum { kSkyMissBit = 1u, kSkyHitBit = 2u, kSkyGroundBit = 4u, kSkySunBit = 8u, kSkyCloudBit = 16u, kSkyFoggedBit = 32u };

// what the launch reads and writes (device pointers; host pointers in the harness)
struct SkyArgs {
    const float* color_in;  // W * H * 3
    const uint32_t* keys;   // W * H
    float* color_out;       // W * H * 3
    uint32_t* fb;           // W * H BGRA8 pixels, or NULL
    uint32_t* summary;      // miss, hit, ground, sun, cloud, fogged, or NULL
    uint32_t W, H;
    uint32_t flags, glow_log2, octaves, seed;
    float zenith[3], horizon[3], ground[3], sun_color[3], cloud_color[3];
    float sun[3];           // s: sun_dir normalised
    float glow_strength, ground_fade, cos_outer, disc_span;  // disc_span = cos_inner - cos_outer
    float cloud_y, cloud_scale, cloud_offset[2], cloud_max_t, cloud_floor /* 1 - cloud_cover */, cloud_sharp, cloud_fade;
    float cloud_top;        // S = 2^(octaves - 1)
    float fog_start, fog_density, fog_max;
};

__host__ __device__ inline float sky_mix(float a, float b, float w) { return a + (b - a) * w; }
__host__ __device__ inline float sky_smooth(float x) { return (x * x) * (3.0f - 2.0f * x); }

// n of the contract, in float as the device would form it: the square root is correctly rounded in both, and taken once, here
inline float sky_sun_norm(const float v[3]) { return __builtin_sqrtf(frame_dot(v, v)); }

// The parameter checks of include/vxrt.h that need neither the context nor a pointer of the call: 0 when all pass, else
// the place of the first that fails in the documented order (2: W or H; 3: params or its struct_size; 4: flags or reserved_;
// 5: a colour; 6: glow_log2 or octaves; 7: a scalar; 8: fog_max or cloud_cover above 1; 9: the cosines; 10: the sun;
// 11: the pose).
inline int sky_frame_check(uint32_t W, uint32_t H, const vxrt_sky_params* p)
{
    if (!denoise_frame_ok(W, H))
        return 2;
    if (!p || p->struct_size != sizeof(vxrt_sky_params))
        return 3;
    if ((p->flags & ~kSkyClouds) != 0u || p->reserved_ != 0)
        return 4;
    const float* const colours[5] = {p->zenith, p->horizon, p->ground, p->sun_color, p->cloud_color};
    for (const float* c : colours)
        for (int k = 0; k < 3; ++k)
            if (!(c[k] >= 0.0f) || !frame_finite(c[k]))
                return 5;
    if (p->glow_log2 > kSkyMaxGlowLog2 || p->octaves < 1u || p->octaves > kSkyMaxOctaves)
        return 6;
    const float scalars[10] = {p->glow_strength, p->ground_fade, p->cloud_scale, p->cloud_max_t, p->cloud_cover,
                               p->cloud_sharp,   p->cloud_fade,  p->fog_start,   p->fog_density, p->fog_max};
    for (float v : scalars)
        if (!(v >= 0.0f) || !frame_finite(v))
            return 7;
    if (!frame_finite(p->cloud_y) || !frame_finite(p->cloud_offset[0]) || !frame_finite(p->cloud_offset[1]))
        return 7;
    if (p->fog_max > 1.0f || p->cloud_cover > 1.0f)
        return 8;
    if (!(p->cos_inner > p->cos_outer) || !(p->cos_outer >= -1.0f) || !(p->cos_inner <= 1.0f))  // (a NaN fails)
        return 9;
    const float n = sky_sun_norm(p->sun_dir);
    if (!(n > 0.0f) || !frame_finite(n))
        return 10;
    return pose_finite(p->cam) ? 0 : 11;
}

// the call's arguments as the launch takes them (params checked before)
inline void sky_frame_args(SkyArgs& A, uint32_t W, uint32_t H, const vxrt_sky_params& p)
{
    A.W = W;
    A.H = H;
    A.flags = p.flags;
    A.glow_log2 = p.glow_log2;
    A.octaves = p.octaves;
    A.seed = p.seed;
    const float n = sky_sun_norm(p.sun_dir);
    for (int k = 0; k < 3; ++k) {
        A.zenith[k] = p.zenith[k];
        A.horizon[k] = p.horizon[k];
        A.ground[k] = p.ground[k];
        A.sun_color[k] = p.sun_color[k];
        A.cloud_color[k] = p.cloud_color[k];
        A.sun[k] = p.sun_dir[k] / n;
    }
    A.glow_strength = p.glow_strength;
    A.ground_fade = p.ground_fade;
    A.cos_outer = p.cos_outer;
    A.disc_span = p.cos_inner - p.cos_outer;
    A.cloud_y = p.cloud_y;
    A.cloud_scale = p.cloud_scale;
    A.cloud_offset[0] = p.cloud_offset[0];
    A.cloud_offset[1] = p.cloud_offset[1];
    A.cloud_max_t = p.cloud_max_t;
    A.cloud_floor = 1.0f - p.cloud_cover;
    A.cloud_sharp = p.cloud_sharp;
    A.cloud_fade = p.cloud_fade;
    A.cloud_top = (float)(1u << (p.octaves - 1u));
    A.fog_start = p.fog_start;
    A.fog_density = p.fog_density;
    A.fog_max = p.fog_max;
}

// base(d) of the contract: the sky behind everything, without disc and clouds; sd = dot(d, s)
__host__ __device__ inline void sky_base(const SkyArgs& A, float h, float sd, float c[3])
{
    if (h >= 0.0f) {
        const float a = 1.0f - h, a2 = a * a, a4 = a2 * a2;
        float g = sd > 0.0f ? sd : 0.0f;
        for (uint32_t i = 0; i < A.glow_log2; ++i)  // (uniform: a kernel argument)
            g = g * g;
        const float k = A.glow_strength * g;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            c[ch] = sky_mix(A.zenith[ch], A.horizon[ch], a4) + A.sun_color[ch] * k;
    } else {
        const float w = frame_clamp01((-h) * A.ground_fade);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            c[ch] = sky_mix(A.horizon[ch], A.ground[ch], w);
    }
}

// value(i, j, k) of the contract: a 32-bit mix of a noise cell and a seed, its upper 24 bits as a float in 0 .. 1
__host__ __device__ inline float sky_value(uint32_t i, uint32_t j, uint32_t k)
{
    uint32_t m = (i * 0x8DA6B343u) ^ (j * 0xD8163841u) ^ (k * 0xCB1AB31Fu);
    m ^= m >> 16;
    m *= 0x7FEB352Du;
    m ^= m >> 15;
    m *= 0x846CA68Bu;
    m ^= m >> 16;
    return (float)(m >> 8) * 5.9604644775390625e-8f;  // 2^-24
}

// vnoise of the contract; |qx|, |qz| < 2^30
__host__ __device__ inline float sky_vnoise(float qx, float qz, uint32_t k)
{
    const float fx = floorf(qx), fz = floorf(qz);
    const uint32_t ix = (uint32_t)(int32_t)fx, iz = (uint32_t)(int32_t)fz;
    const float wx = sky_smooth(qx - fx), wz = sky_smooth(qz - fz);
    const float x0 = sky_mix(sky_value(ix, iz, k), sky_value(ix + 1u, iz, k), wx);
    const float x1 = sky_mix(sky_value(ix, iz + 1u, k), sky_value(ix + 1u, iz + 1u, k), wx);
    return sky_mix(x0, x1, wz);
}

// Where the ray (o, d) of a miss pixel with h = d.y meets the cloud plane, in noise units; false: the pixel has no cloud
__host__ __device__ inline bool sky_cloud_point(const SkyArgs& A, const float o[3], const float d[3], float& px, float& pz)
{
    const float h = d[1];
    if ((A.flags & kSkyClouds) == 0u || !(h > 0.0f) || !(o[1] < A.cloud_y))
        return false;
    const float t = (A.cloud_y - o[1]) / h;
    if (!frame_finite(t) || !(t <= A.cloud_max_t))
        return false;
    px = (o[0] + t * d[0]) * A.cloud_scale + A.cloud_offset[0];
    pz = (o[2] + t * d[2]) * A.cloud_scale + A.cloud_offset[1];
    const float lim = 1073741824.0f, qx = px * A.cloud_top, qz = pz * A.cloud_top;  // 2^30
    return qx > -lim && qx < lim && qz > -lim && qz < lim;  // (a NaN fails)
}

// alpha of the contract at noise point (px, pz) under a ray of height h
__host__ __device__ inline float sky_clouds(const SkyArgs& A, float px, float pz, float h)
{
    float n = 0.0f, freq = 1.0f, amp = 0.5f;
    for (uint32_t i = 0; i < A.octaves; ++i) {  // (uniform: a kernel argument)
        n = n + amp * sky_vnoise(px * freq, pz * freq, A.seed + i);
        freq = freq * 2.0f;
        amp = amp * 0.5f;
    }
    const float dens = frame_clamp01((n - A.cloud_floor) * A.cloud_sharp);
    return dens * frame_clamp01(h * A.cloud_fade);
}

// Pixel (x, y) with primary ray (o, d): its colour and BGRA8 pixel stored; returns the kSky* bits of the counters it adds to.
// The octave loop runs under `cloudy` alone: a wave without a cloud lane branches over it.
__host__ __device__ inline uint32_t sky_pixel(const SkyArgs& A, uint32_t x, uint32_t y, const float o[3], const float d[3])
{
    const uint32_t i = y * A.W + x;  // W * H <= 2^26: every index fits 32 bits
    VXRT_SKY_CHECK(kSkyKeys, i);
    const uint32_t key = A.keys[i];
    const float h = d[1], sd = frame_dot(d, A.sun);
    float c[3];
    sky_base(A, h, sd, c);
    uint32_t bits;
    if (key == 0u) {
        bits = kSkyMissBit | (h < 0.0f ? (uint32_t)kSkyGroundBit : 0u);
        if (h >= 0.0f) {
            const float e = sky_smooth(frame_clamp01((sd - A.cos_outer) / A.disc_span));
            bits |= e > 0.0f ? (uint32_t)kSkySunBit : 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                c[ch] = sky_mix(c[ch], A.sun_color[ch], e);
            float px = 0.0f, pz = 0.0f;
            const bool cloudy = sky_cloud_point(A, o, d, px, pz);
            if (cloudy) {
                const float alpha = sky_clouds(A, px, pz, h);
                bits |= alpha > 0.0f ? (uint32_t)kSkyCloudBit : 0u;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    c[ch] = sky_mix(c[ch], A.cloud_color[ch], alpha);
            }
        }
    } else {
        bits = kSkyHitBit;
        VXRT_SKY_CHECK(kSkyColorIn, 3u * i + 2u);
        const float in[3] = {A.color_in[3u * i], A.color_in[3u * i + 1u], A.color_in[3u * i + 2u]};
        const FrameFace face = frame_face(key);
        float da;
        const float t = frame_plane_t(face.a, face.pl, o, d, da);
        float f = 0.0f;
        if (da != 0.0f && frame_finite(t) && t >= 0.0f) {
            float u = t - A.fog_start;
            u = u > 0.0f ? u : 0.0f;
            const float q = u * A.fog_density;
            f = q / (1.0f + q);
            f = f < A.fog_max ? f : A.fog_max;
        }
        const bool fogged = f > 0.0f;
        bits |= fogged ? (uint32_t)kSkyFoggedBit : 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            c[ch] = fogged ? sky_mix(in[ch], c[ch], f) : in[ch];
    }
    VXRT_SKY_CHECK(kSkyColorOut, 3u * i + 2u);
    frame_store_color(A.color_out, i, c);
    if (A.fb) {
        VXRT_SKY_CHECK(kSkyFb, i);
        A.fb[i] = dn_bgra8(c[0], c[1], c[2]);
    }
    return bits;
}

#ifndef VXRT_HOST_CHECK  // the kernel of vxrt_sky.hip
struct RenderArgs;  // (vxrt_kernels.hpp)
// R carries the camera (camera_args, ortho, origin, fwd, up, right), A the rest; cus: the device's compute units
hipError_t sky_frame(const RenderArgs& R, const SkyArgs& A, uint32_t cus, hipStream_t stream);
#endif

}  // namespace vxrt
