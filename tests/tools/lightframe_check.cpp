// Host harness of the light on frames (voxelengine_amd/csrc/vxrt_light_frame.hpp: the voxel face of a pixel, the nine cells
// in front of it, the corner triples, the position on the face, the interpolation, the colour and the stores), compiled for
// the CPU through tests/tools/hoststub and run workgroup by workgroup and lane by lane.  The world is the oracle's brickmap
// (oracle/vxo_world.c) of a dense grid, laid out as the library holds it in HBM.  The harness restates what
// vxrt_light_frame.hip adds around that code, which the GPU suite covers:
//   the launch      frame_launch.h;
//   the camera      one lane per pixel, its primary ray handed in (the camera is the renderer's, covered on the GPU);
//   the summary     zeroed, then the lanes' results counted.
// Every index the code forms into an input, an output, the cell table, the brick pool or the level bytes is checked against
// that array's size (an array the call was not given has size 0); every array carries a guard behind it.  Run by
// tests/test_light_frame_host.py, which compares with tests/ref_light_frame.py.
//
//   lightframe_check in.bin out.bin
//   in:  i32 0, W, H, io, f, X, Y, Z, box origin[3], box dims[3], flags, outside_level, compute units, 0, 0, 0
//        io: 1 levels given, 2 fb, 4 terms, 8 summary, 16 the colour output is the colour input
//        then 8 f32 sky_floor, block_color[3], ao_curve[4]; X * Y * Z / 32 u32 dense words (vxo_sample_index64); W * H * 3 f32
//        colours; W * H u32 keys; W * H i64 hit indices; W * H * 3 f32 ray origins; W * H * 3 f32 ray directions; (levels) one
//        u8 per voxel of the box in region order
//   out: W * H * 3 f32 colours; (fb) W * H u32 BGRA8; (terms) W * H * 3 f32; (summary) 4 u32
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool check_or_report(int array, uint64_t index);
// an index outside its array ends the run before the access
#define VXRT_LF_CHECK(array, index)                       \
    do {                                                  \
        if (!check_or_report(array, (uint64_t)(index))) { \
            printf("FAILED\n");                           \
            exit(1);                                      \
        }                                                 \
    } while (0)

#include "../../voxelengine_amd/csrc/vxrt_light_frame.hpp"
#include "hbm_world.h"
using namespace vxrt;
#include "frame_launch.h"

static bool check_or_report(int array, uint64_t index)
{
    const int before = fails;
    check_index(array, index);
    return fails == before;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: lightframe_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[20];
    float fl[8];
    if (!in || fread(hd, 4, 20, in) != 20 || fread(fl, 4, 8, in) != 8)
        return 2;
    const uint32_t W = (uint32_t)hd[1], H = (uint32_t)hd[2], io = (uint32_t)hd[3];
    const int f = hd[4], X = hd[5], Y = hd[6], Z = hd[7];
    const bool given = io & 1u, fb = io & 2u, terms = io & 4u, summary = io & 8u, alias = io & 16u;
    vxrt_light_frame_params p{};
    p.struct_size = sizeof p;
    p.flags = (uint32_t)hd[14];
    p.outside_level = (uint32_t)hd[15];
    p.sky_floor = fl[0];
    for (int k = 0; k < 3; ++k) {
        p.block_color[k] = fl[1 + k];
        p.box_origin[k] = hd[8 + k];
        p.box_dims[k] = hd[11 + k];
        p.cam.fwd[k] = p.cam.up[k] = p.cam.right[k] = p.cam.origin[k] = 0.0f;
    }
    for (int k = 0; k < 4; ++k)
        p.ao_curve[k] = fl[4 + k];
    if (light_frame_check(W, H, &p) != 0) {
        printf("outside the contract\n");
        return 2;
    }
    const uint64_t n = (uint64_t)W * H, nvox = (uint64_t)p.box_dims[0] * p.box_dims[1] * p.box_dims[2];
    const uint32_t guard = 0x5A5A5A5Au;
    float guardf;
    memcpy(&guardf, &guard, 4);
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    std::vector<float> cin(3u * n + 1u), cout_(3u * n + 1u, guardf), tv(3u * n + 1u, guardf), o(3u * n), d(3u * n);
    std::vector<uint32_t> keys(n + 1u), fbv(n + 1u, guard), sum(5u, guard);
    std::vector<long long> hit(n + 1u);
    std::vector<uint8_t> levels(nvox + 16u, 0x5A);
    if (fread(dense.data(), 4, dense.size(), in) != dense.size() || fread(cin.data(), 4, 3u * n, in) != 3u * n ||
        fread(keys.data(), 4, n, in) != n || fread(hit.data(), 8, n, in) != n || fread(o.data(), 4, 3u * n, in) != 3u * n ||
        fread(d.data(), 4, 3u * n, in) != 3u * n || (given && fread(levels.data(), 1, nvox, in) != nvox))
        return 2;
    fclose(in);
    cin[3u * n] = guardf;
    keys[n] = guard;
    hit[n] = 0x5A5A5A5A5A5A5A5All;
    const std::vector<float> cin0 = cin;
    const std::vector<uint32_t> keys0 = keys;
    const std::vector<long long> hit0 = hit;
    const std::vector<uint8_t> levels0 = levels;

    // the oracle's brickmap in HBM order
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    if (!w)
        return 2;
    const HbmWorld h = to_hbm(w);
    vxo_world_free(w);
    const CollideWorld Wd = h.world();
    const std::vector<uint2> meta0 = h.meta;
    const std::vector<uint32_t> pool0 = h.pool;

    LightFrameArgs A{};
    light_frame_args(A, W, H, p);
    A.color_in = cin.data();
    A.keys = keys.data();
    A.hit = hit.data();
    A.levels = given ? levels.data() : nullptr;
    A.color_out = alias ? cin.data() : cout_.data();
    A.fb = fb ? fbv.data() : nullptr;
    A.terms = terms ? tv.data() : nullptr;
    A.summary = summary ? sum.data() : nullptr;
    g_size[kLfColorIn] = 3u * n;
    g_size[kLfKeys] = n;
    g_size[kLfHit] = n;
    g_size[kLfLevels] = given ? nvox : 0u;
    g_size[kLfColorOut] = 3u * n;
    g_size[kLfFb] = fb ? n : 0u;
    g_size[kLfTerms] = terms ? 3u * n : 0u;
    g_size[kLfMeta] = h.meta.size();
    g_size[kLfPool] = h.pool.size();

    uint32_t count[4] = {0u, 0u, 0u, 0u};
    frame_launch(W, H, summary, (uint32_t)hd[16], [&](uint32_t x, uint32_t y, uint64_t at) {
        const uint32_t bits = lf_pixel(A, Wd, x, y, &o[3u * at], &d[3u * at]);
        CHECK(bits < 16u && ((bits & kLfHitBit) != 0u || bits == 0u));
        for (int k = 0; k < 4; ++k)
            count[k] += (bits >> k) & 1u;
    });
    if (summary)
        for (int k = 0; k < 4; ++k)
            sum[k] = count[k];

    // guards, and the inputs unchanged (the colours: unless they are the output)
    uint32_t g[3];
    memcpy(&g[0], &cin[3u * n], 4);
    memcpy(&g[1], &cout_[3u * n], 4);
    memcpy(&g[2], &tv[3u * n], 4);
    CHECK(g[0] == guard && g[1] == guard && g[2] == guard && keys[n] == guard && fbv[n] == guard && sum[4] == guard);
    CHECK(keys == keys0 && hit == hit0 && levels == levels0);
    CHECK(memcmp(h.meta.data(), meta0.data(), meta0.size() * sizeof(uint2)) == 0 && h.pool == pool0);
    if (!alias)
        CHECK(memcmp(cin.data(), cin0.data(), 12u * n) == 0);
    if (alias)
        for (uint64_t i = 0; i < 3u * n; ++i)
            CHECK(memcmp(&cout_[i], &guard, 4) == 0);
    if (!fb)
        for (uint64_t i = 0; i < n; ++i)
            CHECK(fbv[i] == guard);
    if (!terms)
        for (uint64_t i = 0; i < 3u * n; ++i)
            CHECK(memcmp(&tv[i], &guard, 4) == 0);
    if (!summary)
        for (int i = 0; i < 4; ++i)
            CHECK(sum[i] == guard);

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(alias ? cin.data() : cout_.data(), 4, 3u * n, out);
    if (fb)
        fwrite(fbv.data(), 4, n, out);
    if (terms)
        fwrite(tv.data(), 4, 3u * n, out);
    if (summary)
        fwrite(sum.data(), 4, 4, out);
    fclose(out);
    printf("%llu indices checked, failures %d\n%s\n", (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
