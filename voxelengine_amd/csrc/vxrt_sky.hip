// vxrt_sky.hip -- sky on frames (include/vxrt.h, vxrt_sky_frame; host side in vxrt_api_query.hip, the per-pixel logic in
// vxrt_sky.hpp).  One frame stage (vxrt_frame_stage.hpp) on the caller's stream:
//
//   k_sky_frame   The colours, the sun and every scalar are kernel arguments: they stay in scalar registers, as do the trip
//                 counts of the glow and the octave loops (glow_log2, octaves), so both loops are uniform.  A miss lane
//                 loads its key alone; the octave loop (four hashes and two smooth weights per octave) runs under the
//                 lanes that have a cloud, and a wave without one branches over it.  The six counters of the summary are
//                 zeroed by k_frame_zero, not by a memset (vxrt_frame_stage.hpp says why).
#include "vxrt_frame_stage.hpp"
#include "vxrt_sky.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_sky_params) == 208 && sizeof(vxrt_sky_summary) == 4u * kSkyCounters, "sky params layout");

__global__ __launch_bounds__(1024) void k_sky_frame(const RenderArgs R, const SkyArgs A)
{
    frame_stage<kSkyCounters>(
        R, A.W, A.H, A.summary, [&](uint32_t x, uint32_t y, const float* o, const float* d) { return sky_pixel(A, x, y, o, d); },
        [](uint32_t bits, uint32_t k) { return ((bits >> k) & 1u) != 0u; });
}

// host entry point (vxrt_api_query.hip): arguments validated there.  Asynchronous on `stream`.
hipError_t sky_frame(const RenderArgs& R, const SkyArgs& A, uint32_t cus, hipStream_t stream)
{
    return frame_stage_launch<kSkyCounters, true>(k_sky_frame, A.W, A.H, A.summary, cus, stream, R, A);
}

}  // namespace vxrt
