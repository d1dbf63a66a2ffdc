// vxrt_reproject.hip -- the temporal filter (include/vxrt.h, vxrt_reproject_frame; host side in vxrt_api_query.hip, the
// per-pixel logic in vxrt_reproject.hpp).  One frame stage (vxrt_frame_stage.hpp) on the caller's stream:
//
//   k_reproject   rp_pixel loads the pixel's colour and key, the four 16-byte history taps and the four key taps of the
//                 previous frame (all eight issued before any is used) and stores one record, one float3 and one BGRA8
//                 pixel.  It returns what became of the pixel, not bits: counter 0 (hit) counts every lane that is no miss,
//                 counter k the lanes whose pixel is k (reused, offscreen, rejected).
#include "vxrt_frame_stage.hpp"
#include "vxrt_reproject.hpp"

namespace vxrt {

static_assert(sizeof(RpRec) == 16 && sizeof(vxrt_history) == 16, "history record");
static_assert(sizeof(vxrt_camera_pose) == 48 && sizeof(vxrt_reproject_params) == 112, "reproject params layout");
static_assert(kRpMiss == 0 && kRpReused == 1 && kRpOffscreen == 2 && kRpRejected == 3 && sizeof(vxrt_reproject_summary) == 16,
              "an idle lane is a miss; counter k counts the pixels that are k");

__global__ __launch_bounds__(1024) void k_reproject(const RenderArgs R, const ReprojectArgs A)
{
    frame_stage<4u>(
        R, A.W, A.H, A.summary, [&](uint32_t x, uint32_t y, const float* o, const float* d) { return rp_pixel(A, x, y, o, d); },
        [](uint32_t what, uint32_t k) { return k == 0u ? what != kRpMiss : what == k; });
}

// host entry point (vxrt_api_query.hip): arguments validated there.  Asynchronous on `stream`.
hipError_t reproject_frame(const RenderArgs& R, const ReprojectArgs& A, uint32_t cus, hipStream_t stream)
{
    return frame_stage_launch<4u, false>(k_reproject, A.W, A.H, A.summary, cus, stream, R, A);
}

}  // namespace vxrt
