// vxrt_material.hip -- voxel materials (include/vxrt.h, vxrt_material_field / vxrt_material_frame; host side in
// vxrt_api_query.hip, the per-lane and per-pixel logic in vxrt_material.hpp).  One launch each on the caller's stream:
//
//   k_material_field  lanes along x, four voxels per lane, a wave per task (x chunk of 256 voxels or 64 / L whole rows of
//                     consecutive z, one y segment), four tasks per workgroup.  A lane marches down its segment from 16 rows
//                     above it with the run above each of its voxels in a register (mat_field_lane); the world comes as the
//                     region layer's row words.  The bytes of a lane and row are one dword store where the row length is a
//                     multiple of four and the output 4-byte aligned, else byte stores.  The summary is tallied in LDS and
//                     leaves the workgroup as one atomic per non-zero counter.
//   k_material_frame  the frame stages' body (frame_stage of vxrt_frame_stage.hpp) written out, as in k_light_frame, on their
//                     launcher (an instance of the body measured level with this form, profiles/frame_stage.md, but the
//                     suite has not run on it): every hit lane walks at most under_depth + 1 voxels up its column through
//                     CollideWorld (mat_pixel), loads one palette entry and at most one texel.  The rules
//                     travel by value in the kernel arguments.
//
// No host synchronisation, no allocation: every byte and every pixel is a pure function of the call's inputs.
#include "../../include/vxrt.h"
#include "vxrt_frame_stage.hpp"
#include "vxrt_material.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_material_band) == 8 && sizeof(vxrt_material_rules) == 100 && sizeof(vxrt_material) == 20, "material rules layout");
static_assert(sizeof(vxrt_material_summary) == 4u * kMatTallyWords && sizeof(vxrt_material_frame_params) == 68 &&
                  sizeof(vxrt_material_frame_summary) == 16,
              "material params layout");

__global__ __launch_bounds__(256) void k_material_field(const MaterialFieldArgs A, const CollideWorld Wd)
{
    __shared__ uint32_t tally[kMatTallyWords];
    for (uint32_t i = threadIdx.x; i < kMatTallyWords; i += 256u)
        tally[i] = 0u;
    __syncthreads();
    const uint64_t task = flat_block() * 4u + (threadIdx.x >> 6);
    if (task < A.tasks)
        mat_field_lane(A, Wd, task, threadIdx.x & 63u, tally);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kMatTallyWords; i += 256u)
        if (tally[i])
            atomicAdd(&A.summary[i], tally[i]);
}

__global__ __launch_bounds__(1024) void k_material_frame(const RenderArgs R, const MaterialFrameArgs A, const CollideWorld Wd)
{
    __shared__ uint32_t counts[kRpCounted / 64u][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, per = blockDim.x >> 6;
    const uint32_t gw = blockIdx.x * per + wave, waves = gridDim.x * per;
    uint32_t n_hit = 0u, n_painted = 0u, n_top = 0u, n_tex = 0u;  // (uniform: the wave's counts)
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
            bits = mat_pixel(A, Wd, x, y, of, df);
        }
        if (A.summary) {  // (uniform; every lane of the wave is here)
            n_hit += (uint32_t)__popcll(__ballot((bits & kMatHitBit) != 0u));
            n_painted += (uint32_t)__popcll(__ballot((bits & kMatPaintedBit) != 0u));
            n_top += (uint32_t)__popcll(__ballot((bits & kMatTopBit) != 0u));
            n_tex += (uint32_t)__popcll(__ballot((bits & kMatTexturedBit) != 0u));
        }
    }
    if (!A.summary)
        return;
    if (lane == 0u) {
        counts[wave][0] = n_hit;
        counts[wave][1] = n_painted;
        counts[wave][2] = n_top;
        counts[wave][3] = n_tex;
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

// host entry points (vxrt_api_query.hip): arguments validated there.  Asynchronous on `stream`.
hipError_t material_field(const MaterialFieldArgs& A, const CollideWorld& Wd, hipStream_t stream)
{
    if (hipError_t e = hipMemsetAsync(A.summary, 0, sizeof(vxrt_material_summary), stream))
        return e;
    hipLaunchKernelGGL(k_material_field, grid_2d((A.tasks + 3u) / 4u), dim3(256), 0, stream, A, Wd);
    return hipGetLastError();
}

hipError_t material_frame(const RenderArgs& R, const MaterialFrameArgs& A, const CollideWorld& Wd, uint32_t cus, hipStream_t stream)
{
    return frame_stage_launch<4u, false>(k_material_frame, A.W, A.H, A.summary, cus, stream, R, A, Wd);
}

}  // namespace vxrt
