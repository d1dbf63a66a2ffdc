// vxrt_frame_stage.hpp -- the one kernel body and the one launcher of the per-pixel frame stages (k_reproject and k_sky_frame; k_light_frame
// and k_material_frame keep bodies of their own, vxrt_light_frame.hip says why); device code; the launch shape is
// vxrt_reproject.hpp's ("launch"), the per-pixel helpers are vxrt_frame.hpp's.
//
//   frame_stage   one lane per pixel, lanes along x, four waves on a tile of 64 x 4 pixels like k_frame_guides.  The pixel's
//                 primary ray comes from the render kernel's own camera_ray (vxrt_camera.hpp, the general instantiation);
//                 the stage's `pixel` does the rest and returns the stage's bits.  Without a summary a workgroup is those
//                 four waves on one tile and no atomic runs.  With one, the N counters are reduced per wave by ballot and
//                 popcount over the wave's tiles (`counted` says which lanes add to which), per workgroup in LDS, and lane k
//                 adds counter k with atomicAdd where it is not zero: few large workgroups, each wave on several tiles
//                 (vxrt_reproject.hpp, "launch", says why).
//   k_frame_zero  the counters of a summary zeroed by one wave in front of the stage's kernel.  The sky stage alone uses it;
//                 the other stages use hipMemsetAsync.  With the memset, a graph captured around a vxrt_sky_frame whose
//                 summary was allocated inside the capture found other bytes than zeros in the counters from its second
//                 replay on (profiles/sky_frame.md).  The cause is not established -- a 24-byte memset node as such is not
//                 it: the distance field's replays correctly -- so this is a workaround, not a diagnosis.
//
// No host synchronisation, no allocation: every pixel is a pure function of the call's inputs.
#pragma once

#include "vxrt_camera.hpp"
#include "vxrt_reproject.hpp"  // the launch shape (and with it vxrt_frame.hpp)

namespace vxrt {

// the primary ray of pixel (x, y) under the camera R carries (camera_args, ortho, origin, fwd, up, right)
__device__ __forceinline__ void frame_ray(const RenderArgs& R, uint32_t x, uint32_t y, float o[3], float d[3])
{
    LaneView V;
    V.origin = R.origin;
    V.fwd = R.fwd;
    V.up = R.up;
    V.right = R.right;
    f3 of, df;
    camera_ray<FrameTraits<false>>(R, V, (int)x, (int)y, of, df);
    o[0] = of.x, o[1] = of.y, o[2] = of.z;
    d[0] = df.x, d[1] = df.y, d[2] = df.z;
}

// pixel(x, y, o, d): the stage's per-pixel code, returns its bits (0 stands for an idle lane: no counter may count it);
// counted(bits, k): whether a lane with those bits adds to counter k of the N of the summary.
template <uint32_t N, class Pixel, class Counted>
__device__ __forceinline__ void frame_stage(const RenderArgs& R, uint32_t W, uint32_t H, uint32_t* summary, const Pixel& pixel,
                                            const Counted& counted)
{
    __shared__ uint32_t counts[kRpCounted / 64u][N];
    // (per: the launch's workgroup by its own rule, rp_block.  Not blockDim.x: inside this body the compiler reads it with a
    // vector load of the 16-bit field and a select on the workgroup's index, in front of every workgroup;
    // profiles/frame_stage.md)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, per = rp_block(summary != nullptr) >> 6;
    const uint32_t gw = blockIdx.x * per + wave, waves = gridDim.x * per;
    uint32_t n[N] = {};  // (uniform: the wave's counts)
    uint32_t x, y;
    for (uint32_t i = 0; rp_wave_pixel(W, H, gw, waves, i, lane, x, y); ++i) {
        uint32_t bits = 0u;
        if (x < W && y < H) {
            float o[3], d[3];
            frame_ray(R, x, y, o, d);
            bits = pixel(x, y, o, d);
        }
        if (summary) {  // (uniform; every lane of the wave is here)
#pragma unroll
            for (uint32_t k = 0; k < N; ++k)
                n[k] += (uint32_t)__popcll(__ballot(counted(bits, k)));
        }
    }
    if (!summary)
        return;
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < N; ++k)
            counts[wave][k] = n[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        uint32_t sum = 0u;
        for (uint32_t w = 0; w < per; ++w)
            sum += counts[w][threadIdx.x];
        if (sum)
            atomicAdd(&summary[threadIdx.x], sum);
    }
}

// (a template, so that only a stage that zeroes by kernel carries it)
template <uint32_t N>
__global__ __launch_bounds__(64) void k_frame_zero(uint32_t* summary)
{
    if (threadIdx.x < N)
        summary[threadIdx.x] = 0u;
}

// The summary's N words zeroed where there is one (by k_frame_zero or by a memset), then `kernel` on the launch shape of a
// W x H frame with `args`.  Asynchronous on `stream`; cus: the device's compute units.
template <uint32_t N, bool ZERO_BY_KERNEL, class Kernel, class... Args>
inline hipError_t frame_stage_launch(Kernel kernel, uint32_t W, uint32_t H, uint32_t* summary, uint32_t cus, hipStream_t stream,
                                     const Args&... args)
{
    if (summary) {
        if constexpr (ZERO_BY_KERNEL) {
            hipLaunchKernelGGL(k_frame_zero<N>, dim3(1), dim3(64), 0, stream, summary);
            if (hipError_t e = hipGetLastError())
                return e;
        } else if (hipError_t e = hipMemsetAsync(summary, 0, N * sizeof(uint32_t), stream)) {
            return e;
        }
    }
    uint32_t block, grid;
    rp_launch_shape(W, H, summary != nullptr, cus, block, grid);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace vxrt
