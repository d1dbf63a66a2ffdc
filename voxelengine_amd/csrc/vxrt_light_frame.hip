// vxrt_light_frame.hip -- light on frames (include/vxrt.h, vxrt_light_frame; host side in vxrt_api_query.hip, the per-pixel
// logic in vxrt_light_frame.hpp).  One launch on the caller's stream, by the frame stages' launcher (vxrt_frame_stage.hpp):
//
//   k_light_frame   Solidity is read through the query layer's world (CollideWorld, vxrt_region.hpp).  Every hit lane makes
//                 the four corner triples of its own face (lf_face: nine cell records, nine brick words, nine level bytes)
//                 and shades (lf_shade).  A form in which the first lane of a run of equal (hit index, key) within the wave
//                 made the corners and the run's other lanes took the thirteen words by shuffle gave the same bits and the
//                 same time within 4 % either way (profiles/light_frame.md): neighbouring lanes' loads of the same cells
//                 already coalesce, and the wave runs lf_face once in both forms.  It was dropped.
//                 The kernel has the frame stages' body (frame_stage of vxrt_frame_stage.hpp) written out: as an instance of the
//                 shared body it measured 0.4 .. 1.4 us of 77 .. 89 slower with a summary at 1080p (profiles/frame_stage.md).
#include "vxrt_frame_stage.hpp"
#include "vxrt_light_frame.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_light_frame_params) == 124 && sizeof(vxrt_light_frame_summary) == 16, "light frame params layout");

__global__ __launch_bounds__(1024) void k_light_frame(const RenderArgs R, const LightFrameArgs A, const CollideWorld Wd)
{
    __shared__ uint32_t counts[kRpCounted / 64u][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, per = blockDim.x >> 6;
    const uint32_t gw = blockIdx.x * per + wave, waves = gridDim.x * per;
    uint32_t n_hit = 0u, n_box = 0u, n_occ = 0u, n_dark = 0u;  // (uniform: the wave's counts)
    uint32_t x, y;
    for (uint32_t i = 0; rp_wave_pixel(A.W, A.H, gw, waves, i, lane, x, y); ++i) {
        uint32_t bits = 0u;
        if (x < A.W && y < A.H) {
            LaneView V;
            V.origin = R.origin;
            V.fwd = R.fwd;
            V.up = R.up;
            V.right = R.right;
            f3 o, d;
            camera_ray<FrameTraits<false>>(R, V, (int)x, (int)y, o, d);
            const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
            bits = lf_pixel(A, Wd, x, y, of, df);
        }
        if (A.summary) {  // (uniform; every lane of the wave is here)
            n_hit += (uint32_t)__popcll(__ballot((bits & kLfHitBit) != 0u));
            n_box += (uint32_t)__popcll(__ballot((bits & kLfHitBit) != 0u && (bits & kLfInBoxBit) != 0u));
            n_occ += (uint32_t)__popcll(__ballot((bits & kLfHitBit) != 0u && (bits & kLfOccludedBit) != 0u));
            n_dark += (uint32_t)__popcll(__ballot((bits & kLfDarkBit) != 0u));
        }
    }
    if (!A.summary)
        return;
    if (lane == 0u) {
        counts[wave][0] = n_hit;
        counts[wave][1] = n_box;
        counts[wave][2] = n_occ;
        counts[wave][3] = n_dark;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        uint32_t n = 0u;
        for (uint32_t w = 0; w < per; ++w)
            n += counts[w][threadIdx.x];
        if (n)
            atomicAdd(&A.summary[threadIdx.x], n);
    }
}

// host entry point (vxrt_api_query.hip): arguments validated there.  Asynchronous on `stream`.
hipError_t light_frame(const RenderArgs& R, const LightFrameArgs& A, const CollideWorld& Wd, uint32_t cus, hipStream_t stream)
{
    return frame_stage_launch<4u, false>(k_light_frame, A.W, A.H, A.summary, cus, stream, R, A, Wd);
}

}  // namespace vxrt
