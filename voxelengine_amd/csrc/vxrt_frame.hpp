// vxrt_frame.hpp -- what the per-pixel frame stages share (include/vxrt.h: vxrt_reproject_frame, vxrt_light_frame,
// vxrt_material_frame, vxrt_sky_frame): the small float helpers, the check of a camera pose, the fields of a guide key, the
// parameter of a primary ray at a face plane, the colour store.  Host and device: the
// stages' per-pixel headers include it, and with them the host side in vxrt_api_query.hip and the host harnesses of the tests
// (through tests/tools/hoststub).  The launch shape of the stages is vxrt_reproject.hpp's ("launch"); the shared kernel body and
// the launcher are device code and live in vxrt_frame_stage.hpp.
//
// Frame.  W x H pixels, x fastest, the denoiser's limits (denoise_frame_ok).  A lane owns one pixel: it reads its own inputs
// and writes its own outputs, so no pixel reads what another writes and the colour output may be the colour input.  The
// primary ray (o, d) of the pixel is an input of every stage's per-pixel code: camera_ray (vxrt_camera.hpp) votes across the
// wave and stays with the kernel (frame_ray of vxrt_frame_stage.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vxrt.h"
#include "vxrt_denoise.hpp"  // the frame limits (denoise_frame_ok, kDnMaxAxis), dn_bgra8

namespace vxrt {

// (the frame_ prefix: <math.h> declares a finite() of its own)
__host__ __device__ inline bool frame_finite(float x) { return x - x == 0.0f; }  // (x - x: 0 for a finite x, NaN otherwise)
__host__ __device__ inline float frame_clamp01(float x) { return x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x; }
__host__ __device__ inline float frame_dot(const float u[3], const float v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// every component of a camera pose finite (a refusal of every stage)
inline bool pose_finite(const vxrt_camera_pose& p)
{
    for (int k = 0; k < 3; ++k)
        if (!frame_finite(p.origin[k]) || !frame_finite(p.fwd[k]) || !frame_finite(p.up[k]) || !frame_finite(p.right[k]))
            return false;
    return true;
}

// The face a guide key (guide_key of vxrt_denoise.hpp) names: its axis, the side it is seen from and its plane.  The axis
// is clamped to 2, so that whatever word stands in a key buffer indexes nothing out of range.  The temporal filter, which
// read the axis unclamped ("a guide key has a <= 2"), takes this decode too: every use of the axis, here and in the stages,
// is one of the selects a == 0, a == 1 and a >= 2, and the clamp changes none of the three.
struct FrameFace {
    uint32_t a;
    bool toward;
    float pl;
};

__host__ __device__ inline FrameFace frame_face(uint32_t key)
{
    FrameFace F;
    F.a = (key >> 26) & 31u;
    F.a = F.a > 2u ? 2u : F.a;
    F.toward = (key >> 25) & 1u;
    F.pl = (float)(key & 0x1FFFFFFu);
    return F;
}

// The parameter t at which the ray (o, d) meets the plane pl of axis a, and da, the ray's component along that axis (t is
// no position where da == 0 or t is not finite: the caller looks).  Selects, not indexing: the vectors stay in registers.
__host__ __device__ inline float frame_plane_t(uint32_t a, float pl, const float o[3], const float d[3], float& da)
{
    const float oa = a == 0u ? o[0] : a == 1u ? o[1] : o[2];
    da = a == 0u ? d[0] : a == 1u ? d[1] : d[2];
    return (pl - oa) / da;
}

// Pixel i's colour into the colour output.  The index check of a stage's harness (VXRT_*_CHECK) stays in front of the call,
// with that stage's array id; so does the one line of the BGRA8 store (dn_bgra8), under the stage's own test of `fb`.
__host__ __device__ inline void frame_store_color(float* color_out, uint32_t i, const float c[3])
{
    color_out[3u * i] = c[0];
    color_out[3u * i + 1u] = c[1];
    color_out[3u * i + 2u] = c[2];
}

}  // namespace vxrt
