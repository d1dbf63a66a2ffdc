// The launch of a frame stage (voxelengine_amd/csrc/vxrt_frame_stage.hpp), restated for the host harnesses of the stages:
// rp_launch_shape's workgroups, every lane of every workgroup on the pixels rp_wave_pixel gives its wave, lanes outside
// the frame idle.  Checks the launch shape and that every pixel of the frame is visited exactly once; `pixel(x, y, at)` is the
// harness's own per-pixel work (at = y * W + x).  The includer has CHECK and the namespace vxrt in scope.
#pragma once

#include <cstdint>
#include <vector>

template <class PixelFn>
static void frame_launch(uint32_t W, uint32_t H, bool summary, uint32_t cus, PixelFn pixel)
{
    uint32_t block = 0u, grid = 0u;
    rp_launch_shape(W, H, summary, cus, block, grid);
    CHECK(grid >= 1u && block == rp_block(summary) && (summary || grid == rp_tiles(W, H)));
    CHECK(!summary || grid <= (cus ? cus : 1u) * kRpCountedPerCu);
    const uint32_t per = rp_block(summary) >> 6, waves = grid * per;  // (as frame_stage takes it, not from `block`)
    const uint64_t n = (uint64_t)W * H;
    uint64_t pixels = 0;
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t b = 0; b < grid; ++b)
        for (uint32_t tid = 0; tid < block; ++tid) {
            uint32_t x, y;
            for (uint32_t i = 0; rp_wave_pixel(W, H, b * per + (tid >> 6), waves, i, tid & 63u, x, y); ++i) {
                if (x >= W || y >= H)
                    continue;
                const uint64_t at = (uint64_t)y * W + x;
                CHECK(!seen[at]);
                seen[at] = 1;
                pixel(x, y, at);
                ++pixels;
            }
        }
    CHECK(pixels == n);
}
