// vxrt_pixel_map.hpp -- the persistent render kernel's map from a launch coordinate to a frame pixel and to a row of the
// destination buffers (framebuffer, colour AOV, hit AOV, accumulation history).  A header of its own, needing nothing but
// RenderArgs, so that tests/tools/pixel_map_check.cpp can walk it on the host; included by vxrt_persist2.hpp.
// (k_render in vxrt_kernels.hip keeps its own, independently written copy: variant 1 is the cross-check.)
#pragma once

#include "vxrt_kernels.hpp"

namespace vxrt {

struct PixelCoords {
    uint32_t tx, ty;  // launch coordinates of the reference's thread (crosshair, RNG seed)
    int x, y;         // frame pixel
    int out_row;      // row in the destination buffers
    bool live;
};

// The launch-uniform frame flags as the persistent render kernel reads them.  COMMON: the plain shaded frame -- shaded mode,
// perspective camera, no checkerboard, no strips (hence no packed rows), no accumulation history, no hit-index AOV -- for
// which launch_is_common (vxrt_kernels.hip) picks the kernel's COMMON instantiations: every flag is a constant there and the
// code behind it is not compiled.  Otherwise the flags are the launch's arguments.  (shadow, bounce_samples, bounce_all_hits,
// the colour AOV and the hand-out orders stay run-time values in both.)
template <bool COMMON>
struct FrameTraits {
    static __host__ __device__ __forceinline__ int mode(const RenderArgs& A) { return COMMON ? 0 : A.mode; }
    static __host__ __device__ __forceinline__ bool ortho(const RenderArgs& A) { return COMMON ? false : A.ortho != 0; }
    static __host__ __device__ __forceinline__ bool checkerboard(const RenderArgs& A) { return COMMON ? false : A.checkerboard != 0; }
    static __host__ __device__ __forceinline__ bool sharded(const RenderArgs& A) { return COMMON ? false : A.strip_count > 1; }
    static __host__ __device__ __forceinline__ bool compact(const RenderArgs& A) { return COMMON ? false : A.compact != 0; }
    static __host__ __device__ __forceinline__ bool accum(const RenderArgs& A) { return COMMON ? false : A.accum != nullptr; }
    // a launch's hit-index AOV: some view has one (multi-view: want_hit_aov), and a view's own pointer
    static __host__ __device__ __forceinline__ bool want_hit_aov(const RenderArgs& A, bool multi)
    {
        return COMMON ? false : (multi ? A.want_hit_aov != 0 : A.hit_aov != nullptr);
    }
    static __host__ __device__ __forceinline__ long long* hit_aov(long long* p) { return COMMON ? nullptr : p; }
};

// launch (tx,row) -> pixel (Renderer.cu:183-196 + this build's strip sharding)
template <bool COMMON = false>
__host__ __device__ __forceinline__ PixelCoords pixel_coords(const RenderArgs& A, uint32_t frame_number, uint32_t tx, uint32_t row)
{
    using FT = FrameTraits<COMMON>;
    PixelCoords c;
    c.tx = tx;
    c.ty = row;
    c.x = (int)tx;
    const bool sharded = FT::sharded(A);
    if (sharded && !FT::checkerboard(A)) {
        // A shard's launch rows are its own frame rows in order: launch row = packed row, the frame row follows from
        // the strip arithmetic, and ownership holds by construction -- no division by the strip count, and none by the
        // strip height when it is a power of two (strip_shift >= 0; the default 16 is).
        const uint32_t sr = (uint32_t)A.strip_rows;
        const uint32_t q = A.strip_shift >= 0 ? row >> A.strip_shift : row / sr;
        c.ty = (q * (uint32_t)A.strip_count + (uint32_t)A.strip_index) * sr + (row - q * sr);
        c.y = (int)c.ty;
        c.live = row < A.launch_rows && (uint32_t)c.x < A.width && (uint32_t)c.y < A.height;
        c.out_row = FT::compact(A) ? (int)row : c.y;
        return c;
    }
    c.live = row < A.launch_rows;
    c.y = (int)c.ty;
    if (FT::checkerboard(A)) {
        c.y *= 2;
        if ((c.x % 2) == 0)
            c.y += 1;
        if (frame_number % 2 == 0)
            c.y += 1;
    }
    c.live = c.live && (uint32_t)c.x < A.width && (uint32_t)c.y < A.height;
    if (c.live && sharded && ((uint32_t)c.y / (uint32_t)A.strip_rows) % (uint32_t)A.strip_count != (uint32_t)A.strip_index)
        c.live = false;
    c.out_row = c.y;
    if (FT::compact(A) && sharded)
        c.out_row = (int)((((uint32_t)c.y / (uint32_t)A.strip_rows) / (uint32_t)A.strip_count) * (uint32_t)A.strip_rows +
                          (uint32_t)c.y % (uint32_t)A.strip_rows);
    return c;
}

}  // namespace vxrt
