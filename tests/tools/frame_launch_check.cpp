// The walk of a frame stage's launch (tests/tools/frame_launch.h over voxelengine_amd/csrc/vxrt_reproject.hpp) on the edge shapes:
// frames narrower, as wide as and wider than a tile on both axes, and frames one pixel thin of the longest side, on one
// compute unit and on 256, with and without a summary.  frame_launch checks the launch shape (grid == tiles without a summary,
// 1 <= grid <= 2 * cus with one) and that every pixel is visited exactly once; a lane outside the frame does nothing there, as in the
// kernel body.
// Run by tests/test_frame_launch_host.py.   stdout: launches walked, "ALL OK" or "FAILED"
#include <cstdio>

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (fails < 20)                                         \
                printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                \
        }                                                           \
    } while (0)

#include "../../voxelengine_amd/csrc/vxrt_reproject.hpp"
using namespace vxrt;
#include "frame_launch.h"

int main()
{
    const uint32_t side[4][2] = {{1u, 1u}, {63u, 3u}, {64u, 4u}, {65u, 5u}}, cus[2] = {1u, 256u};
    uint32_t frames[18][2], nf = 0u, launches = 0u;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            frames[nf][0] = side[i][0], frames[nf++][1] = side[j][1];
    frames[nf][0] = 65535u, frames[nf++][1] = 1u;
    frames[nf][0] = 1u, frames[nf++][1] = 65535u;
    for (uint32_t f = 0; f < nf; ++f)
        for (int c = 0; c < 2; ++c)
            for (int summary = 0; summary < 2; ++summary, ++launches) {
                const uint32_t W = frames[f][0], H = frames[f][1];
                frame_launch(W, H, summary != 0, cus[c], [](uint32_t, uint32_t, uint64_t) {});
            }
    printf("%u launches walked, failures %d\n%s\n", launches, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
