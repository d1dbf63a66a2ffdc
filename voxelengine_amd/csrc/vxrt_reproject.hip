// vxrt_reproject.hip -- the temporal filter (include/vxrt.h, vxrt_reproject_frame; host side in vxrt_api_query.hip, the
// per-pixel logic in vxrt_reproject.hpp).  One launch on the caller's stream:
//
//   k_reproject   one lane per pixel, lanes along x, four waves on a tile of 64 x 4 pixels like k_frame_guides.  The
//                 pixel's primary ray comes from the render kernel's own camera_ray (vxrt_camera.hpp, the general
//                 instantiation), rp_pixel does the rest: the pixel's colour and key, the four 16-byte history taps and
//                 the four key taps of the previous frame (all eight issued before any is used), one record, one float3
//                 and one BGRA8 store.  Without a summary a workgroup is those four waves on one tile and no atomic runs.
//                 With one, the counters are reduced per wave by ballot and popcount over the wave's tiles, per workgroup
//                 in LDS, and one lane adds those that are not zero with atomicAdd: few large workgroups, each wave on
//                 several tiles (vxrt_reproject.hpp, "launch", says why).
//
// No host synchronisation, no allocation: every pixel is a pure function of the call's inputs.
#include "../../include/vxrt.h"
#include "vxrt_camera.hpp"
#include "vxrt_reproject.hpp"

namespace vxrt {

static_assert(sizeof(RpRec) == 16 && sizeof(vxrt_history) == 16, "history record");
static_assert(sizeof(vxrt_camera_pose) == 48 && sizeof(vxrt_reproject_params) == 112, "reproject params layout");

__global__ __launch_bounds__(1024) void k_reproject(const RenderArgs R, const ReprojectArgs A)
{
    __shared__ uint32_t counts[kRpCounted / 64u][3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, per = blockDim.x >> 6;
    const uint32_t gw = blockIdx.x * per + wave, waves = gridDim.x * per;
    uint32_t reused = 0u, offscreen = 0u, rejected = 0u;  // (uniform: the wave's counts)
    uint32_t x, y;
    for (uint32_t i = 0; rp_wave_pixel(A.W, A.H, gw, waves, i, lane, x, y); ++i) {
        uint32_t what = kRpMiss;
        if (x < A.W && y < A.H) {
            LaneView V;
            V.origin = R.origin;
            V.fwd = R.fwd;
            V.up = R.up;
            V.right = R.right;
            f3 o, d;
            camera_ray<FrameTraits<false>>(R, V, (int)x, (int)y, o, d);
            const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
            what = rp_pixel(A, x, y, of, df);
        }
        if (A.summary) {  // (uniform; every lane of the wave is here)
            reused += (uint32_t)__popcll(__ballot(what == kRpReused));
            offscreen += (uint32_t)__popcll(__ballot(what == kRpOffscreen));
            rejected += (uint32_t)__popcll(__ballot(what == kRpRejected));
        }
    }
    if (!A.summary)
        return;
    if (lane == 0u) {
        counts[wave][0] = reused;
        counts[wave][1] = offscreen;
        counts[wave][2] = rejected;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        reused = offscreen = rejected = 0u;
        for (uint32_t w = 0; w < per; ++w) {
            reused += counts[w][0];
            offscreen += counts[w][1];
            rejected += counts[w][2];
        }
        if (reused + offscreen + rejected)
            atomicAdd(&A.summary[0], reused + offscreen + rejected);
        if (reused)
            atomicAdd(&A.summary[1], reused);
        if (offscreen)
            atomicAdd(&A.summary[2], offscreen);
        if (rejected)
            atomicAdd(&A.summary[3], rejected);
    }
}

// host entry point (vxrt_api_query.hip): arguments validated there.  Asynchronous on `stream`.
hipError_t reproject_frame(const RenderArgs& R, const ReprojectArgs& A, uint32_t cus, hipStream_t stream)
{
    if (A.summary)
        if (hipError_t e = hipMemsetAsync(A.summary, 0, 4u * sizeof(uint32_t), stream))
            return e;
    uint32_t block, grid;
    rp_launch_shape(A.W, A.H, A.summary != nullptr, cus, block, grid);
    hipLaunchKernelGGL(k_reproject, dim3(grid), dim3(block), 0, stream, R, A);
    return hipGetLastError();
}

}  // namespace vxrt
