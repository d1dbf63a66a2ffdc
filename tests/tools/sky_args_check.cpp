// Host check of the argument limits of the sky on frames (voxelengine_amd/csrc/vxrt_sky.hpp: sky_frame_check,
// sky_frame_args), compiled for the CPU through tests/tools/hoststub.  No device: every parameter check at the first value
// refused and the last accepted, and the documented order of the refusals -- each call has the earlier faults mended and all
// the later ones still in it.  The checks that need the context or a pointer of the call (a NULL ctx, the NULL buffers) are
// the GPU suite's.  Run by tests/test_sky_host.py.
//
//   sky_args_check
//   stdout: cases checked, "ALL OK" or "FAILED"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../voxelengine_amd/csrc/vxrt_sky.hpp"
using namespace vxrt;

static int fails = 0;
static uint64_t cases = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        ++cases;                                                    \
        if (!(c)) {                                                 \
            if (fails < 20)                                         \
                printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                \
        }                                                           \
    } while (0)

// every value at the end of its range that is still accepted
static vxrt_sky_params good()
{
    vxrt_sky_params p{};
    p.struct_size = sizeof p;
    p.flags = VXRT_SKY_CLOUDS;
    p.glow_log2 = 8u;
    p.octaves = 6u;
    p.seed = 0xFFFFFFFFu;
    for (int k = 0; k < 3; ++k) {
        p.zenith[k] = 0.0f;
        p.horizon[k] = 3.0e38f;
        p.ground[k] = p.sun_color[k] = p.cloud_color[k] = 1.0f;
        p.cam.fwd[k] = -3.0e38f;
    }
    p.sun_dir[1] = 1.0e-19f;  // (its square is a denormal: n > 0 still)
    p.glow_strength = p.ground_fade = p.cloud_scale = p.cloud_max_t = p.cloud_sharp = p.cloud_fade = p.fog_start = p.fog_density = 3.0e38f;
    p.cloud_cover = p.fog_max = 1.0f;
    p.cos_inner = 1.0f;
    p.cos_outer = -1.0f;
    p.cloud_y = -3.0e38f;
    p.cloud_offset[0] = 3.0e38f;
    p.cloud_offset[1] = -3.0e38f;
    return p;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(vxrt_sky_params) == 208 && sizeof(vxrt_sky_summary) == 24, "params layout");
    CHECK(sky_frame_check(1u, 1u, nullptr) == 3);
    const vxrt_sky_params ok = good();
    CHECK(sky_frame_check(16u, 8u, &ok) == 0);
    // the frame limits (the denoiser's)
    const uint32_t frames[][3] = {{1, 1, 1}, {65535, 1, 1}, {1, 65535, 1}, {8192, 8192, 1}, {65535, 1024, 1}, {0, 8, 0}, {8, 0, 0},
                                  {65536, 1, 0}, {1, 65536, 0}, {8193, 8192, 0}, {65535, 1025, 0}};
    for (const auto& fr : frames)
        CHECK((sky_frame_check(fr[0], fr[1], &ok) == 0) == (fr[2] != 0u) && (fr[2] != 0u || sky_frame_check(fr[0], fr[1], &ok) == 2));

    // every later fault in place; mended one by one, in the documented order
    vxrt_sky_params p = good();
    p.struct_size -= 4u;
    p.flags = 2u;
    p.ground[1] = -1.0f;
    p.octaves = 7u;
    p.fog_start = nan;
    p.fog_max = 1.5f;
    p.cos_outer = 1.0f;
    p.sun_dir[1] = 0.0f;
    p.cam.up[1] = inf;
    CHECK(sky_frame_check(0u, 8u, &p) == 2);
    CHECK(sky_frame_check(16u, 8u, nullptr) == 3);
    CHECK(sky_frame_check(16u, 8u, &p) == 3);
    p.struct_size = sizeof p + 4u;
    CHECK(sky_frame_check(16u, 8u, &p) == 3);
    p.struct_size = sizeof p;
    CHECK(sky_frame_check(16u, 8u, &p) == 4);
    for (uint32_t flags : {2u, 3u, 4u, 0x80000000u, 0xFFFFFFFFu}) {
        p.flags = flags;
        CHECK(sky_frame_check(16u, 8u, &p) == 4);
    }
    p.flags = 0u;
    p.reserved_ = -1;
    CHECK(sky_frame_check(16u, 8u, &p) == 4);
    p.reserved_ = 0;
    CHECK(sky_frame_check(16u, 8u, &p) == 5);
    p.ground[1] = 0.0f;
    for (int k = 0; k < 15; ++k)
        for (float v : {nan, inf, -inf, -1.0e-30f}) {
            vxrt_sky_params q = p;
            (&q.zenith[0])[k] = v;  // zenith, horizon, ground, sun_color and cloud_color lie one behind the other
            CHECK(sky_frame_check(16u, 8u, &q) == 5);
        }
    CHECK(&p.cloud_color[2] - &p.zenith[0] == 14);
    CHECK(sky_frame_check(16u, 8u, &p) == 6);
    for (uint32_t o : {0u, 7u, 0xFFFFFFFFu}) {
        p.octaves = o;
        CHECK(sky_frame_check(16u, 8u, &p) == 6);
    }
    p.octaves = 1u;
    for (uint32_t g : {9u, 0xFFFFFFFFu}) {
        p.glow_log2 = g;
        CHECK(sky_frame_check(16u, 8u, &p) == 6);
    }
    p.glow_log2 = 0u;
    CHECK(sky_frame_check(16u, 8u, &p) == 7);
    p.fog_start = 0.0f;
    float vxrt_sky_params::* const scalars[] = {&vxrt_sky_params::glow_strength, &vxrt_sky_params::ground_fade, &vxrt_sky_params::cloud_scale,
                                                &vxrt_sky_params::cloud_max_t,   &vxrt_sky_params::cloud_cover, &vxrt_sky_params::cloud_sharp,
                                                &vxrt_sky_params::cloud_fade,    &vxrt_sky_params::fog_start,   &vxrt_sky_params::fog_density,
                                                &vxrt_sky_params::fog_max};
    for (auto m : scalars)
        for (float v : {nan, inf, -inf, -1.0e-30f}) {
            vxrt_sky_params q = p;
            q.*m = v;
            CHECK(sky_frame_check(16u, 8u, &q) == 7);
        }
    for (float v : {nan, inf, -inf}) {
        vxrt_sky_params q = p;
        q.cloud_y = v;
        CHECK(sky_frame_check(16u, 8u, &q) == 7);
        q = p;
        q.cloud_offset[0] = v;
        CHECK(sky_frame_check(16u, 8u, &q) == 7);
        q = p;
        q.cloud_offset[1] = v;
        CHECK(sky_frame_check(16u, 8u, &q) == 7);
    }
    CHECK(sky_frame_check(16u, 8u, &p) == 8);
    p.fog_max = 1.0f;
    p.cloud_cover = std::nextafter(1.0f, 2.0f);
    CHECK(sky_frame_check(16u, 8u, &p) == 8);
    p.cloud_cover = 1.0f;
    p.fog_max = std::nextafter(1.0f, 2.0f);
    CHECK(sky_frame_check(16u, 8u, &p) == 8);
    p.fog_max = 0.0f;
    CHECK(sky_frame_check(16u, 8u, &p) == 9);
    const float cosines[][3] = {{1.0f, -1.0f, 1}, {0.5f, 0.25f, 1}, {std::nextafter(-1.0f, 0.0f), -1.0f, 1}, {1.0f, std::nextafter(1.0f, 0.0f), 1},
                                {0.5f, 0.5f, 0}, {0.25f, 0.5f, 0}, {std::nextafter(1.0f, 2.0f), 0.5f, 0}, {0.5f, std::nextafter(-1.0f, -2.0f), 0},
                                {nan, 0.5f, 0}, {0.5f, nan, 0}, {inf, 0.0f, 0}, {0.0f, -inf, 0}};
    for (const auto& c : cosines) {
        vxrt_sky_params q = p;
        q.cos_inner = c[0];
        q.cos_outer = c[1];
        q.sun_dir[1] = 1.0f;
        q.cam.up[1] = 0.0f;
        CHECK(sky_frame_check(16u, 8u, &q) == (c[2] != 0.0f ? 0 : 9));
    }
    p.cos_outer = 0.5f;
    CHECK(sky_frame_check(16u, 8u, &p) == 10);
    const float suns[][4] = {{0, 1, 0, 1}, {1.0e-19f, 0, 0, 1}, {1.0e19f, 1.0e19f, 0, 1}, {0, 0, 0, 0}, {-0.0f, 0, -0.0f, 0}, {1.0e-30f, 0, 0, 0},
                             {2.0e19f, 0, 0, 0}, {nan, 1, 0, 0}, {0, inf, 0, 0}, {0, 1, -inf, 0}};
    for (const auto& s : suns) {
        vxrt_sky_params q = p;
        for (int k = 0; k < 3; ++k)
            q.sun_dir[k] = s[k];
        q.cam.up[1] = 0.0f;
        CHECK(sky_frame_check(16u, 8u, &q) == (s[3] != 0.0f ? 0 : 10));
    }
    p.sun_dir[1] = 1.0f;
    CHECK(sky_frame_check(16u, 8u, &p) == 11);
    p.cam.up[1] = 0.0f;
    for (int k = 0; k < 12; ++k)
        for (float v : {nan, inf, -inf}) {
            vxrt_sky_params q = p;
            (&q.cam.origin[0])[k] = v;
            CHECK(sky_frame_check(16u, 8u, &q) == 11);
        }
    CHECK(sky_frame_check(16u, 8u, &p) == 0);

    // what the launch takes is what the call gave
    SkyArgs A{};
    vxrt_sky_params q = good();
    q.sun_dir[0] = 0.0f;
    q.sun_dir[1] = 3.0f;
    q.sun_dir[2] = 4.0f;
    q.cloud_cover = 0.25f;
    q.cos_inner = 0.75f;
    q.cos_outer = 0.5f;
    q.octaves = 5u;
    sky_frame_args(A, 16u, 8u, q);
    CHECK(A.W == 16u && A.H == 8u && A.flags == VXRT_SKY_CLOUDS && A.glow_log2 == 8u && A.octaves == 5u && A.seed == 0xFFFFFFFFu);
    CHECK(A.sun[0] == 0.0f && A.sun[1] == 3.0f / 5.0f && A.sun[2] == 4.0f / 5.0f && A.cloud_floor == 0.75f && A.disc_span == 0.25f && A.cloud_top == 16.0f);
    CHECK(A.horizon[2] == 3.0e38f && A.zenith[0] == 0.0f && A.cloud_color[1] == 1.0f && A.cloud_y == -3.0e38f && A.cloud_offset[1] == -3.0e38f);
    CHECK(A.fog_max == 1.0f && A.fog_start == 3.0e38f && A.cos_outer == 0.5f && A.glow_strength == 3.0e38f);
    // the noise: the value of a cell lies in 0 .. 1 - 2^-24, wraps with the cell and differs between seeds
    CHECK(sky_value(0u, 0u, 0u) == 0.0f);
    float lo = 1.0f, hi = 0.0f;
    for (uint32_t i = 0; i < 4096u; ++i) {
        const float v = sky_value(i * 2654435761u, i ^ 0xABCDu, i >> 3);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    CHECK(lo >= 0.0f && lo < 0.01f && hi > 0.99f && hi <= 1.0f - 5.9604644775390625e-8f);
    CHECK(sky_value(0xFFFFFFFFu + 1u, 5u, 1u) == sky_value(0u, 5u, 1u) && sky_value(3u, 5u, 1u) != sky_value(3u, 5u, 2u));
    // at a cell corner the noise is the corner's value; in the middle of a cell the mean of the four
    CHECK(sky_vnoise(3.0f, -2.0f, 9u) == sky_value(3u, (uint32_t)-2, 9u));
    const float m = sky_vnoise(3.5f, -1.5f, 9u);
    const float x0 = sky_mix(sky_value(3u, (uint32_t)-2, 9u), sky_value(4u, (uint32_t)-2, 9u), 0.5f);
    const float x1 = sky_mix(sky_value(3u, (uint32_t)-1, 9u), sky_value(4u, (uint32_t)-1, 9u), 0.5f);
    CHECK(m == sky_mix(x0, x1, 0.5f) && sky_smooth(0.5f) == 0.5f && sky_smooth(0.0f) == 0.0f && sky_smooth(1.0f) == 1.0f);
    printf("%llu cases, failures %d\n%s\n", (unsigned long long)cases, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
