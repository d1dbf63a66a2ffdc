// vxrt_denoise.hip -- the edge-avoiding frame denoiser (include/vxrt.h, vxrt_frame_guides / vxrt_denoise_frame; host side in
// vxrt_api.hip, the shared logic in vxrt_denoise.hpp).  The launches of the two calls, all on the caller's stream:
//
//   k_frame_guides      one lane per pixel, lanes along x: the pixel's primary ray from the render kernel's own camera_ray
//                       (vxrt_camera.hpp, the general instantiation: the camera kind is the launch's flag) and the hit
//                       index give the face key.  Reads the hit AOV, writes the keys; no world table.
//   k_denoise<STAGED>   one a-trous iteration (vxrt_denoise.hpp).  DIRECT: a wave on 64 consecutive pixels of a row, 25
//                       taps of one 16-byte record each, every tap row a contiguous 1 KB.  STAGED: 64 x 16 pixels and
//                       their halo in LDS first, taps from there.  The first iteration packs (it reads the float3 colours
//                       and the keys), the last one unpacks (float3 and BGRA8 stores): one launch per iteration and
//                       nothing else, unless a single iteration would read the buffer it writes (see denoise_frame).
//
// No atomics, no host synchronisation, no allocation: every pixel is a pure function of the iteration's input.
#include "../../include/vxrt.h"
#include "vxrt_denoise.hpp"
#include "vxrt_frame_stage.hpp"  // frame_ray

#include <cstdlib>

namespace vxrt {

static_assert(sizeof(DnRec) == 16, "workspace record");
static_assert(sizeof(vxrt_denoise_params) == 16, "denoise params layout");

__global__ __launch_bounds__(256) void k_frame_guides(const RenderArgs A, uint32_t* __restrict__ keys, uint32_t Z)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= A.width || y >= A.height)
        return;
    float o[3], d[3];
    frame_ray(A, x, y, o, d);
    const uint64_t i = (uint64_t)y * A.width + x;
    keys[i] = guide_key(A.hit_aov[i], (uint32_t)A.W.X, (uint32_t)A.W.Y, Z, o, d);
}

template <bool STAGED, bool FIRST>
__global__ __launch_bounds__(256) void k_denoise(const DenoiseArgs A)
{
    __shared__ DnRec tile[STAGED ? kDnLdsRecords : 1u];
    if (STAGED) {
        dn_stage<FIRST>(A, blockIdx.x, blockIdx.y, threadIdx.x, tile);
        __syncthreads();
    }
    dn_compute<STAGED, FIRST>(A, blockIdx.x, blockIdx.y, threadIdx.x, tile);
}

template <bool STAGED>
static void dn_launch(const DenoiseArgs& A, bool first, hipStream_t stream)
{
    uint32_t gx, gy;
    dn_grid(A.W, A.H, STAGED, gx, gy);
    if (first)
        hipLaunchKernelGGL((k_denoise<STAGED, true>), dim3(gx, gy), dim3(256), 0, stream, A);
    else
        hipLaunchKernelGGL((k_denoise<STAGED, false>), dim3(gx, gy), dim3(256), 0, stream, A);
}

// the records of a frame from its float3 colours and keys: the pack on its own (denoise_frame says when)
__global__ __launch_bounds__(256) void k_denoise_pack(const DenoiseArgs A)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x < A.W && y < A.H)
        A.dst[y * A.W + x] = dn_load<true>(A, x, y);
}

// host entry point (vxrt_api.hip): arguments validated there; R carries the camera of the frame (camera_args of
// vxrt_api.hip), the hit AOV and the world's X and Y.  Asynchronous on `stream`.
hipError_t frame_guides(const RenderArgs& R, uint32_t Z, uint32_t* keys, hipStream_t stream)
{
    hipLaunchKernelGGL(k_frame_guides, dim3((R.width + 63u) / 64u, (R.height + 3u) / 4u), dim3(256), 0, stream, R, keys, Z);
    return hipGetLastError();
}

// Which instantiation an iteration of step `step` runs: the one that measured faster (profiles/denoise.md).
static bool dn_staged(uint32_t step)
{
    // a mask of steps: bit 0 = step 1, bit 1 = step 2.  Measured at 1080p on the bench frame (profiles/denoise.md): step 1,
    // which packs, 40 us STAGED against 84 DIRECT (the float3 input is read once, not 25 times); step 2 equal without the
    // colour stop (29 us) and 42 against 76 with it.
    uint32_t staged_steps = 3u;
#ifdef VXRT_EXPERIMENTS
    if (const char* e = getenv("VXRT_DENOISE_STAGED"))  // tools/denoise_probe.py: the steps that run STAGED, as that mask
        staged_steps = (uint32_t)atoi(e);
#endif
    return step <= kDnMaxStagedStep && (staged_steps & step) != 0u;
}

// host entry point (vxrt_api.hip): arguments validated there.  Asynchronous on `stream`.
hipError_t denoise_frame(uint32_t W, uint32_t H, const float* color_in, const uint32_t* keys, int32_t iterations, float k,
                         void* work, float* color_out, void* fb, hipStream_t stream)
{
    DnRec* const buf[2] = {(DnRec*)work, (DnRec*)work + (uint64_t)W * H};
    DenoiseArgs A{};
    A.color_in = color_in;
    A.keys = keys;
    A.color_out = color_out;
    A.fb = (uint32_t*)fb;
    A.W = W;
    A.H = H;
    A.k = k;
    // A single iteration reads its neighbours' input while other lanes store their output: when the two buffers overlap,
    // the pack runs as a launch of its own and the iteration reads the workspace.
    const uintptr_t in0 = (uintptr_t)color_in, out0 = (uintptr_t)color_out, bytes = (uintptr_t)W * H * 12u;
    bool packed = false;
    if (iterations == 1 && in0 < out0 + bytes && out0 < in0 + bytes) {
        A.dst = buf[1];
        hipLaunchKernelGGL(k_denoise_pack, dim3((W + 63u) / 64u, (H + 3u) / 4u), dim3(256), 0, stream, A);
        packed = true;
    }
    for (int32_t i = 0; i < iterations; ++i) {
        A.step = 1u << i;
        A.last = i == iterations - 1;
        A.src = buf[(i + 1) & 1];
        A.dst = buf[i & 1];
        if (dn_staged(A.step))
            dn_launch<true>(A, i == 0 && !packed, stream);
        else
            dn_launch<false>(A, i == 0 && !packed, stream);
    }
    return hipGetLastError();
}

}  // namespace vxrt
