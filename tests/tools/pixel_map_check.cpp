// Host harness of the persistent render kernel's pixel map (voxelengine_amd/csrc/vxrt_pixel_map.hpp: pixel_coords).  Fills
// RenderArgs for one launch the way render_launch does (vxrt_api.hip: launch_rows, strip_shift, compact), walks every (tx, row)
// of the launch's padded tile grid -- ceil(W/8)*8 by ceil(launch_rows/8)*8, what the tile queue hands to the lanes -- and
// prints the live pixels; tests/test_frame_shapes_host.py holds them to the model of tests/frame_shape_cases.py.
// PIXEL_MAP_HEADER: the header under test (the test also builds changed copies of it, which this harness must catch).
// build: g++ -O1 -std=c++17 -Itests/tools/hoststub -Ivoxelengine_amd/csrc tests/tools/pixel_map_check.cpp
// usage: pixel_map_check W H strip_rows strip_count strip_index compact checkerboard frame_number
// output: "launch_rows R strip_shift S", then "x y ty out_row" per live pixel in walk order, then "ALL OK"
#include <hip/hip_runtime.h>
#ifndef PIXEL_MAP_HEADER
#define PIXEL_MAP_HEADER "vxrt_pixel_map.hpp"
#endif
#include PIXEL_MAP_HEADER
#include <cstdio>
#include <cstdlib>
using namespace vxrt;

// vxrt_compact_rows (vxrt_api.hip)
static uint32_t compact_rows(uint32_t height, int32_t strip_rows, int32_t strip_count, int32_t strip_index)
{
    if (strip_rows <= 0 || strip_count <= 1)
        return height;
    uint32_t rows = 0;
    const uint32_t nstrips = (height + (uint32_t)strip_rows - 1) / (uint32_t)strip_rows;
    for (uint32_t s = (uint32_t)strip_index; s < nstrips; s += (uint32_t)strip_count) {
        const uint32_t begin = s * (uint32_t)strip_rows;
        const uint32_t end = begin + (uint32_t)strip_rows < height ? begin + (uint32_t)strip_rows : height;
        rows += end - begin;
    }
    return rows;
}

int main(int argc, char** argv)
{
    if (argc < 9) {
        printf("usage: pixel_map_check W H strip_rows strip_count strip_index compact checkerboard frame_number\n");
        return 2;
    }
    static RenderArgs A;  // (zero-initialised, as render_launch's memset leaves it)
    A.width = (uint32_t)atoll(argv[1]);
    A.height = (uint32_t)atoll(argv[2]);
    const int strip_rows = atoi(argv[3]), strip_count = atoi(argv[4]);
    A.strip_rows = strip_rows > 0 ? strip_rows : 16;
    A.strip_count = strip_count > 1 ? strip_count : 1;
    A.strip_index = atoi(argv[5]);
    A.compact = atoi(argv[6]) ? 1 : 0;
    A.checkerboard = atoi(argv[7]) ? 1 : 0;
    const uint32_t frame_number = (uint32_t)atoll(argv[8]);
    A.frame_number = frame_number;
    A.strip_shift = -1;
    for (int b = 0; b < 31; ++b)
        if (A.strip_rows == (1 << b))
            A.strip_shift = b;
    if (A.checkerboard)
        A.launch_rows = A.height >> 1;
    else if (A.strip_count > 1)
        A.launch_rows = compact_rows(A.height, A.strip_rows, A.strip_count, A.strip_index);
    else
        A.launch_rows = A.height;
    printf("launch_rows %u strip_shift %d\n", A.launch_rows, A.strip_shift);
    // (launch_render starts nothing for an empty grid)
    const uint32_t gw = (A.width + 7u) / 8u * 8u, gh = (A.launch_rows + 7u) / 8u * 8u;
    for (uint32_t row = 0; row < gh; ++row)
        for (uint32_t tx = 0; tx < gw; ++tx) {
            const PixelCoords c = pixel_coords(A, frame_number, tx, row);
            if (c.live)
                printf("%d %d %u %d\n", c.x, c.y, c.ty, c.out_row);
        }
    printf("ALL OK\n");
    return 0;
}
