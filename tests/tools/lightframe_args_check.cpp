// Host check of the argument limits of the light on frames (voxelengine_amd/csrc/vxrt_light_frame.hpp: light_frame_check,
// light_frame_args), compiled for the CPU through tests/tools/hoststub.  No world and no device: every parameter check at the
// first value refused and the last accepted, and the documented order of the refusals -- each call has the earlier faults
// mended and all the later ones still in it.  The checks that need the context or a pointer of the call (a NULL ctx, the
// NULL buffers, the world) are the GPU suite's.  Run by tests/test_light_frame_host.py.
//
//   lightframe_args_check
//   stdout: cases checked, "ALL OK" or "FAILED"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../voxelengine_amd/csrc/vxrt_light_frame.hpp"
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

static vxrt_light_frame_params good()
{
    vxrt_light_frame_params p{};
    p.struct_size = sizeof p;
    p.flags = VXRT_LF_SMOOTH | VXRT_LF_OCCLUSION;
    p.outside_level = 0xFFu;
    p.sky_floor = 1.0f;
    for (int k = 0; k < 3; ++k) {
        p.block_color[k] = 0.0f;
        p.box_dims[k] = 1;
        p.box_origin[k] = INT32_MAX - 1;
        p.cam.fwd[k] = -3.0e38f;
    }
    for (int k = 0; k < 4; ++k)
        p.ao_curve[k] = 3.0e38f;
    return p;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(vxrt_light_frame_params) == 124, "params layout");
    CHECK(light_frame_check(1u, 1u, nullptr) == 3);
    const vxrt_light_frame_params ok = good();
    CHECK(light_frame_check(16u, 8u, &ok) == 0);
    // the frame limits (the denoiser's)
    const uint32_t frames[][3] = {{1, 1, 1}, {65535, 1, 1}, {1, 65535, 1}, {8192, 8192, 1}, {65535, 1024, 1}, {0, 8, 0}, {8, 0, 0},
                                  {65536, 1, 0}, {1, 65536, 0}, {8193, 8192, 0}, {65535, 1025, 0}};
    for (const auto& fr : frames)
        CHECK((light_frame_check(fr[0], fr[1], &ok) == 0) == (fr[2] != 0u) && (fr[2] != 0u || light_frame_check(fr[0], fr[1], &ok) == 2));

    // every later fault in place; mended one by one, in the documented order
    vxrt_light_frame_params p = good();
    p.struct_size -= 4u;
    p.flags = 4u;
    p.sky_floor = nan;
    p.ao_curve[3] = -1.0f;
    p.cam.up[1] = inf;
    p.box_dims[2] = 0;
    CHECK(light_frame_check(0u, 8u, &p) == 2);
    CHECK(light_frame_check(16u, 8u, nullptr) == 3);
    CHECK(light_frame_check(16u, 8u, &p) == 3);
    p.struct_size = sizeof p;
    CHECK(light_frame_check(16u, 8u, &p) == 4);
    for (uint32_t flags : {4u, 7u, 8u, 0x80000000u, 0xFFFFFFFFu}) {
        p.flags = flags;
        CHECK(light_frame_check(16u, 8u, &p) == 4);
    }
    p.flags = 0u;
    p.outside_level = 0x100u;
    CHECK(light_frame_check(16u, 8u, &p) == 4);
    p.outside_level = 0xFFu;
    p.reserved_ = 1;
    CHECK(light_frame_check(16u, 8u, &p) == 4);
    p.reserved_ = 0;
    CHECK(light_frame_check(16u, 8u, &p) == 5);
    for (float s : {nan, -inf, inf, -1.0e-30f, std::nextafter(1.0f, 2.0f)}) {
        p.sky_floor = s;
        CHECK(light_frame_check(16u, 8u, &p) == 5);
    }
    for (float s : {0.0f, -0.0f, 1.0f, 0.5f}) {
        p.sky_floor = s;
        CHECK(light_frame_check(16u, 8u, &p) == 6);
    }
    p.ao_curve[3] = 1.0f;
    for (int k = 0; k < 7; ++k)
        for (float v : {nan, inf, -inf, -1.0e-30f}) {
            vxrt_light_frame_params q = p;
            (k < 3 ? q.block_color[k] : q.ao_curve[k - 3]) = v;
            CHECK(light_frame_check(16u, 8u, &q) == 6);
        }
    CHECK(light_frame_check(16u, 8u, &p) == 7);
    p.cam.up[1] = 0.0f;
    for (int k = 0; k < 12; ++k)
        for (float v : {nan, inf, -inf}) {
            vxrt_light_frame_params q = p;
            (&q.cam.origin[0])[k] = v;
            CHECK(light_frame_check(16u, 8u, &q) == 7);
        }
    CHECK(light_frame_check(16u, 8u, &p) == 8);
    // the box: 1 <= dims[k], the product <= 2^28, origin + dims <= 2^31 - 1
    const int32_t dims[][4] = {{1, 1, 1, 1}, {1 << 28, 1, 1, 1}, {1 << 10, 1 << 10, 1 << 8, 1}, {1 << 14, 1, 1 << 14, 1}, {0, 1, 1, 0}, {1, -1, 1, 0},
                               {1, 1, 0, 0}, {(1 << 28) + 1, 1, 1, 0}, {1 << 10, 1 << 10, (1 << 8) + 1, 0}, {INT32_MAX, INT32_MAX, INT32_MAX, 0},
                               {1 << 16, 1 << 16, 1 << 16, 0}, {INT32_MIN, 1, 1, 0}};
    for (const auto& d : dims) {
        vxrt_light_frame_params q = p;
        for (int k = 0; k < 3; ++k) {
            q.box_dims[k] = d[k];
            q.box_origin[k] = 0;
        }
        CHECK(light_frame_check(16u, 8u, &q) == (d[3] ? 0 : 8));
    }
    for (int k = 0; k < 3; ++k)
        for (int32_t d : {1, 5, 1 << 20}) {
            vxrt_light_frame_params q = p;
            q.box_dims[0] = q.box_dims[1] = q.box_dims[2] = 1;
            q.box_dims[k] = d;
            q.box_origin[0] = q.box_origin[1] = q.box_origin[2] = INT32_MIN;
            CHECK(light_frame_check(16u, 8u, &q) == 0);
            q.box_origin[k] = INT32_MAX - d;
            CHECK(light_frame_check(16u, 8u, &q) == 0);
            q.box_origin[k] = INT32_MAX - d + 1;
            CHECK(light_frame_check(16u, 8u, &q) == 8);
        }
    // what the launch takes is what the call gave
    LightFrameArgs A{};
    vxrt_light_frame_params q = good();
    q.box_origin[1] = -7;
    q.box_dims[2] = 9;
    q.block_color[2] = 0.5f;
    light_frame_args(A, 16u, 8u, q);
    CHECK(A.W == 16u && A.H == 8u && A.flags == q.flags && A.outside_level == 0xFFu && A.sky_floor == 1.0f && A.block_color[2] == 0.5f);
    CHECK(A.ao_curve[0] == 3.0e38f && A.ao_curve[3] == 3.0e38f && A.bo[1] == -7 && A.bd[2] == 9 && A.bo[0] == INT32_MAX - 1);
    printf("%llu cases, failures %d\n%s\n", (unsigned long long)cases, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
