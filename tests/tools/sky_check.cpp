// Host harness of the sky on frames (voxelengine_amd/csrc/vxrt_sky.hpp: the sky without disc and clouds, the disc, the cloud
// noise, the fog of a hit pixel and the stores), compiled for the CPU through tests/tools/hoststub and run workgroup by
// workgroup and lane by lane.  The harness restates what vxrt_sky.hip adds around that code, which the GPU suite covers:
//   the launch      frame_launch.h;
//   the camera      one lane per pixel, its primary ray handed in (the camera is the renderer's, covered on the GPU);
//   the summary     zeroed, then the lanes' results counted.
// Every index the code forms into an input or an output is checked against that array's size (an array the call was not
// given has size 0); every array carries a guard behind it.  Run by tests/test_sky_host.py, which compares with
// tests/ref_sky.py.
//
//   sky_check in.bin out.bin
//   in:  i32 0, W, H, io, compute units, 0, 0, 0
//        io: 1 fb, 2 summary, 4 the colour output is the colour input
//        then the 208 bytes of a vxrt_sky_params; W * H * 3 f32 colours; W * H u32 keys; W * H * 3 f32 ray origins;
//        W * H * 3 f32 ray directions
//   out: W * H * 3 f32 colours; (fb) W * H u32 BGRA8; (summary) 6 u32
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t g_size[8], checked = 0;
static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (fails < 20)                                         \
                printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                \
        }                                                           \
    } while (0)
// an index outside its array ends the run before the access
#define VXRT_SKY_CHECK(array, index)                                                                                        \
    do {                                                                                                                    \
        ++checked;                                                                                                          \
        if ((uint64_t)(index) >= g_size[array]) {                                                                           \
            printf("index %llu outside array %d of %llu\nFAILED\n", (unsigned long long)(index), (int)(array),              \
                   (unsigned long long)g_size[array]);                                                                      \
            exit(1);                                                                                                        \
        }                                                                                                                   \
    } while (0)

#include "../../voxelengine_amd/csrc/vxrt_sky.hpp"
using namespace vxrt;
#include "frame_launch.h"

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: sky_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[8];
    vxrt_sky_params p;
    static_assert(sizeof p == 208, "params layout");
    if (!in || fread(hd, 4, 8, in) != 8 || fread(&p, 1, sizeof p, in) != sizeof p)
        return 2;
    const uint32_t W = (uint32_t)hd[1], H = (uint32_t)hd[2], io = (uint32_t)hd[3], cus = (uint32_t)hd[4];
    const bool fb = io & 1u, summary = io & 2u, alias = io & 4u;
    if (sky_frame_check(W, H, &p) != 0) {
        printf("outside the contract: %d\n", sky_frame_check(W, H, &p));
        return 2;
    }
    const uint64_t n = (uint64_t)W * H;
    const uint32_t guard = 0x5A5A5A5Au;
    float guardf;
    memcpy(&guardf, &guard, 4);
    std::vector<float> cin(3u * n + 1u), cout_(3u * n + 1u, guardf), o(3u * n), d(3u * n);
    std::vector<uint32_t> keys(n + 1u), fbv(n + 1u, guard), sum(kSkyCounters + 1u, guard);
    if (fread(cin.data(), 4, 3u * n, in) != 3u * n || fread(keys.data(), 4, n, in) != n || fread(o.data(), 4, 3u * n, in) != 3u * n ||
        fread(d.data(), 4, 3u * n, in) != 3u * n)
        return 2;
    fclose(in);
    cin[3u * n] = guardf;
    keys[n] = guard;
    const std::vector<float> cin0 = cin;
    const std::vector<uint32_t> keys0 = keys;

    SkyArgs A{};
    sky_frame_args(A, W, H, p);
    A.color_in = cin.data();
    A.keys = keys.data();
    A.color_out = alias ? cin.data() : cout_.data();
    A.fb = fb ? fbv.data() : nullptr;
    A.summary = summary ? sum.data() : nullptr;
    g_size[kSkyColorIn] = 3u * n;
    g_size[kSkyKeys] = n;
    g_size[kSkyColorOut] = 3u * n;
    g_size[kSkyFb] = fb ? n : 0u;

    uint32_t count[kSkyCounters] = {0u, 0u, 0u, 0u, 0u, 0u};
    frame_launch(W, H, summary, cus, [&](uint32_t x, uint32_t y, uint64_t at) {
        const uint32_t bits = sky_pixel(A, x, y, &o[3u * at], &d[3u * at]);
        const bool miss = bits & kSkyMissBit, hit = bits & kSkyHitBit;
        CHECK(bits < 64u && miss != hit && (miss || !(bits & (kSkyGroundBit | kSkySunBit | kSkyCloudBit))) && (hit || !(bits & kSkyFoggedBit)));
        for (uint32_t k = 0; k < kSkyCounters; ++k)
            count[k] += (bits >> k) & 1u;
    });
    if (summary)
        for (uint32_t k = 0; k < kSkyCounters; ++k)
            sum[k] = count[k];

    // guards, and the inputs unchanged (the colours: unless they are the output)
    uint32_t g[2];
    memcpy(&g[0], &cin[3u * n], 4);
    memcpy(&g[1], &cout_[3u * n], 4);
    CHECK(g[0] == guard && g[1] == guard && keys[n] == guard && fbv[n] == guard && sum[kSkyCounters] == guard);
    CHECK(keys == keys0);
    if (!alias)
        CHECK(memcmp(cin.data(), cin0.data(), 12u * n) == 0);
    if (alias)
        for (uint64_t i = 0; i < 3u * n; ++i)
            CHECK(memcmp(&cout_[i], &guard, 4) == 0);
    if (!fb)
        for (uint64_t i = 0; i < n; ++i)
            CHECK(fbv[i] == guard);
    if (!summary)
        for (uint32_t i = 0; i < kSkyCounters; ++i)
            CHECK(sum[i] == guard);

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(alias ? cin.data() : cout_.data(), 4, 3u * n, out);
    if (fb)
        fwrite(fbv.data(), 4, n, out);
    if (summary)
        fwrite(sum.data(), 4, kSkyCounters, out);
    fclose(out);
    printf("%llu indices checked, failures %d\n%s\n", (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
