// vxrt_camera.hpp -- the primary ray of a frame pixel (getRayDirection / getRayDirectionOrtho, VoxelRT/Renderer.cu:44-70) as the
// render kernel takes it (vxrt_persist2.hpp), in a header of its own, needing nothing but RenderArgs and FrameTraits, so that
// the guide kernel of the frame denoiser (vxrt_denoise.hip) forms the very same ray from the very same code.
#pragma once

#include "vxrt_kernels.hpp"
#include "vxrt_pixel_map.hpp"

namespace vxrt {

// the per-view inputs of one lane's pixel: kernel arguments for a single-view launch, loaded from the launch's
// ViewArgs array for a multi-view one
struct LaneView {
    f3 origin, fwd, up, right;
    uint32_t frame_number;
    uint8_t* fb;
    float* color_aov;
    long long* hit_aov;
};

// getRayDirection / getRayDirectionOrtho (Renderer.cu:44-70)
// (FT: the launch's frame flags as the kernel reads them, FrameTraits -- the camera kind is a constant in the COMMON instantiations)
template <class FT>
__device__ __forceinline__ void camera_ray(const RenderArgs& A, const LaneView& V, int x, int y, f3& origin, f3& ray)
{
    // (x / W and y / H: small integers over small integers, by the host's reciprocals and one correction step -- exact for
    // every such pair, tests/tools/exact_div_check.c)
    const float u = div_rn((float)x, (float)(int)A.width, A.inv_width), v = div_rn((float)y, (float)(int)A.height, A.inv_height);
    origin = V.origin;
    if (FT::ortho(A)) {
        ray = V.fwd;
        origin = origin + ((V.right * (u * 2 - 1)) * A.ortho_x) * A.ratio;
        origin = origin + (V.up * (v * 2 - 1)) * A.ortho_y;
    } else {
        float su = u * 2 - 1, sv = v * 2 - 1;
        ray.x = V.fwd.x + su * A.kx * V.right.x + sv * A.ky * V.up.x;
        ray.y = V.fwd.y + su * A.kx * V.right.y + sv * A.ky * V.up.y;
        ray.z = V.fwd.z + su * A.kx * V.right.z + sv * A.ky * V.up.z;
        const float dd = dot3(ray, ray);
        const f3 plain = ray;
        ray = unit3_ordinary(plain, dd);
        if (__ballot(!ordinary(dd)) != 0ull)
            ray = unit3(plain);
    }
}

// the ray origin alone (perspective: the camera; ortho: per pixel) -- what shading and the debug view need of a
// pixel's camera ray once the primary ray has been traced
template <class FT>
__device__ __forceinline__ f3 camera_origin(const RenderArgs& A, const LaneView& V, int x, int y)
{
    f3 origin = V.origin;
    if (FT::ortho(A)) {
        const float u = div_rn((float)x, (float)(int)A.width, A.inv_width), v = div_rn((float)y, (float)(int)A.height, A.inv_height);
        origin = origin + ((V.right * (u * 2 - 1)) * A.ortho_x) * A.ratio;
        origin = origin + (V.up * (v * 2 - 1)) * A.ortho_y;
    }
    return origin;
}

}  // namespace vxrt
