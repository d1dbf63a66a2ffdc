// vxrt_sky.hip -- sky on frames (include/vxrt.h, vxrt_sky_frame; host side in vxrt_api_query.hip, the per-pixel logic in
// vxrt_sky.hpp).  One launch on the caller's stream:
//
//   k_sky_frame   one lane per pixel, lanes along x, the launch shape of k_reproject (vxrt_reproject.hpp): four waves on a
//                 tile of 64 x 4 pixels without a summary; with one, few large workgroups whose waves walk several tiles,
//                 count by ballot and popcount, add up in LDS and issue one set of atomics per workgroup.  The pixel's
//                 primary ray comes from the render kernel's own camera_ray (vxrt_camera.hpp, the general instantiation).
//                 The colours, the sun and every scalar are kernel arguments: they stay in scalar registers, as do the trip
//                 counts of the glow and the octave loops (glow_log2, octaves), so both loops are uniform.  A miss lane
//                 loads its key alone; the octave loop (four hashes and two smooth weights per octave) runs under the
//                 lanes that have a cloud, and a wave without one branches over it.
//   k_sky_zero    the six counters of the summary zeroed by one wave in front of k_sky_frame.  A kernel, not a
//                 hipMemsetAsync as in the other frame stages: with the memset, a graph captured around a call whose summary
//                 was allocated inside the capture found other bytes than zeros in the counters from its second replay on
//                 (profiles/sky_frame.md).  The cause is not established -- a 24-byte memset node as such is not it: the
//                 distance field's replays correctly -- so this is a workaround, not a diagnosis.
//
// No host synchronisation, no allocation: every pixel is a pure function of the call's inputs.
#include "../../include/vxrt.h"
#include "vxrt_camera.hpp"
#include "vxrt_sky.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_sky_params) == 208 && sizeof(vxrt_sky_summary) == 4u * kSkyCounters, "sky params layout");

__global__ __launch_bounds__(1024) void k_sky_frame(const RenderArgs R, const SkyArgs A)
{
    __shared__ uint32_t counts[kRpCounted / 64u][kSkyCounters];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, per = blockDim.x >> 6;
    const uint32_t gw = blockIdx.x * per + wave, waves = gridDim.x * per;
    uint32_t n[kSkyCounters] = {0u, 0u, 0u, 0u, 0u, 0u};  // (uniform: the wave's counts)
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
            bits = sky_pixel(A, x, y, of, df);
        }
        if (A.summary) {  // (uniform; every lane of the wave is here)
#pragma unroll
            for (uint32_t k = 0; k < kSkyCounters; ++k)
                n[k] += (uint32_t)__popcll(__ballot(((bits >> k) & 1u) != 0u));
        }
    }
    if (!A.summary)
        return;
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < kSkyCounters; ++k)
            counts[wave][k] = n[k];
    }
    __syncthreads();
    if (threadIdx.x < kSkyCounters) {
        uint32_t sum = 0u;
        for (uint32_t w = 0; w < per; ++w)
            sum += counts[w][threadIdx.x];
        if (sum)
            atomicAdd(&A.summary[threadIdx.x], sum);
    }
}

__global__ __launch_bounds__(64) void k_sky_zero(uint32_t* summary)
{
    if (threadIdx.x < kSkyCounters)
        summary[threadIdx.x] = 0u;
}

// host entry point (vxrt_api_query.hip): arguments validated there.  Asynchronous on `stream`.
hipError_t sky_frame(const RenderArgs& R, const SkyArgs& A, uint32_t cus, hipStream_t stream)
{
    if (A.summary) {
        hipLaunchKernelGGL(k_sky_zero, dim3(1), dim3(64), 0, stream, A.summary);
        if (hipError_t e = hipGetLastError())
            return e;
    }
    uint32_t block, grid;
    rp_launch_shape(A.W, A.H, A.summary != nullptr, cus, block, grid);
    hipLaunchKernelGGL(k_sky_frame, dim3(grid), dim3(block), 0, stream, R, A);
    return hipGetLastError();
}

}  // namespace vxrt
