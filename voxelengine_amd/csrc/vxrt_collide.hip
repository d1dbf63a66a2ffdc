// vxrt_collide.hip -- batched box collision queries against the resident brickmap (include/vxrt.h, vxrt_move_boxes /
// vxrt_overlap_boxes; host side in vxrt_api.hip, the per-body logic in vxrt_collide.hpp).
//
//   k_move_boxes     one lane per body: validation, then the three axis moves of move_body.  x: one row word masked to the
//                    open slabs answers 32 slabs; y / z: slabs nearest first, any nonzero masked word of the cross-section
//                    blocks.  A typical body (1 x 2 x 1 voxels, |delta| of a few voxels) needs a dozen row words.
//   k_overlap_boxes  one lane per body: the popcount of the masked row words of its box.
// Bodies are independent: each lane writes its own results, no atomics, and the result does not depend on the grid.
// Every gather is region_row_word on ranges clipped to the world first, so no load leaves the tables.  The mapping and its
// costs are measured in profiles/r07_collide.md.
#include "../../include/vxrt.h"
#include "vxrt_collide.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_body) == 36, "body layout");

__global__ __launch_bounds__(256) void k_move_boxes(const CollideWorld W, const float* __restrict__ bodies, uint64_t n,
                                                    int o0, int o1, int o2, float* __restrict__ lohi,
                                                    uint32_t* __restrict__ flags)
{
    const int order[3] = {o0, o1, o2};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float b[9], out[6];
        for (int k = 0; k < 9; ++k)
            b[k] = bodies[i * 9 + k];
        const uint32_t fl = collide_move_one(W, b, order, out);
        for (int k = 0; k < 6; ++k)
            lohi[i * 6 + k] = out[k];
        if (flags)
            flags[i] = fl;
    }
}

__global__ __launch_bounds__(256) void k_overlap_boxes(const CollideWorld W, const float* __restrict__ bodies, uint64_t n,
                                                       uint32_t* __restrict__ counts, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float b[9];
        for (int k = 0; k < 9; ++k)
            b[k] = bodies[i * 9 + k];
        uint32_t fl = 0u;
        counts[i] = collide_overlap_one(W, b, fl);
        if (flags)
            flags[i] = fl;
    }
}

// up to 64 K workgroups of 256 lanes; a grid-stride loop covers larger batches
static unsigned collide_blocks(uint64_t n)
{
    const uint64_t b = (n + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : (b ? b : 1));
}

// host entry points (vxrt_api.hip); n > 0
hipError_t move_boxes(const CollideWorld& W, const float* bodies, uint64_t n, const int order[3], float* lohi, uint32_t* flags,
                      hipStream_t stream)
{
    hipLaunchKernelGGL(k_move_boxes, dim3(collide_blocks(n)), dim3(256), 0, stream, W, bodies, n, order[0], order[1], order[2],
                       lohi, flags);
    return hipGetLastError();
}

hipError_t overlap_boxes(const CollideWorld& W, const float* bodies, uint64_t n, uint32_t* counts, uint32_t* flags,
                         hipStream_t stream)
{
    hipLaunchKernelGGL(k_overlap_boxes, dim3(collide_blocks(n)), dim3(256), 0, stream, W, bodies, n, counts, flags);
    return hipGetLastError();
}

}  // namespace vxrt
