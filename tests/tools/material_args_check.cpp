// Host check of the argument limits of the voxel materials (voxelengine_amd/csrc/vxrt_material.hpp: material_rules_check,
// material_paint_ok, material_box_check, material_frame_check, material_field_args), compiled for the CPU through
// tests/tools/hoststub.  No world and no device: every parameter check at the first value refused and the last accepted, and
// the documented order of the refusals -- each call has the earlier faults mended and all the later ones still in it.  The
// checks that need the context or a pointer of the call (a NULL ctx, the NULL buffers, the world) are the GPU suite's.  Run
// by tests/test_material_host.py.
//
//   material_args_check
//   stdout: cases checked, "ALL OK" or "FAILED"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../voxelengine_amd/csrc/vxrt_material.hpp"
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

static vxrt_material_rules good_rules()
{
    vxrt_material_rules r{};
    r.struct_size = sizeof r;
    r.n_bands = 8u;
    for (int i = 0; i < 8; ++i) {
        r.bands[i].y_from = i == 0 ? INT32_MIN : i == 7 ? INT32_MAX : INT32_MIN + i;
        r.bands[i].top = 255u;
        r.bands[i].under = 1u;
        r.bands[i].deep = 255u;
        r.bands[i].under_depth = i & 1 ? 15u : 0u;
    }
    for (int k = 0; k < 3; ++k) {
        r.paint_dims[k] = 1;
        r.paint_origin[k] = INT32_MAX - 1;
    }
    return r;
}

static vxrt_material_frame_params good_params()
{
    vxrt_material_frame_params p{};
    p.struct_size = sizeof p;
    p.n_tiles = 4096u;
    p.tile_shift = 6u;
    for (int k = 0; k < 3; ++k)
        p.cam.fwd[k] = -3.0e38f;
    return p;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(vxrt_material_rules) == 100 && sizeof(vxrt_material_frame_params) == 68 && sizeof(vxrt_material) == 20 &&
                      sizeof(vxrt_material_summary) == 1040,
                  "layouts");
    // ---- the rules ----
    const vxrt_material_rules ok = good_rules();
    CHECK(material_rules_check(&ok) == 0 && material_paint_ok(ok));
    CHECK(material_rules_check(nullptr) == 1);
    vxrt_material_rules r = good_rules();
    r.struct_size += 4u;
    r.n_bands = 9u;
    r.bands[3].top = 0u;
    r.reserved_ = 1;
    r.paint_dims[1] = 0;
    CHECK(material_rules_check(&r) == 1);
    r.struct_size = sizeof r;
    CHECK(material_rules_check(&r) == 2);
    for (uint32_t n : {0u, 9u, 0xFFFFFFFFu}) {
        r.n_bands = n;
        CHECK(material_rules_check(&r) == 2);
    }
    r.n_bands = 8u;
    CHECK(material_rules_check(&r) == 3);
    r.bands[3].top = 1u;
    CHECK(material_rules_check(&r) == 4);
    r.reserved_ = 0;
    CHECK(material_rules_check(&r) == 0 && !material_paint_ok(r));  // (the paint box is looked at only with paint)
    // a band: y_from, the ids, under_depth; bands behind n_bands are not looked at
    for (int i = 0; i < 8; ++i) {
        vxrt_material_rules q = ok;
        q.bands[i].top = 0u;
        CHECK(material_rules_check(&q) == 3);
        q = ok;
        q.bands[i].under = 0u;
        CHECK(material_rules_check(&q) == 3);
        q = ok;
        q.bands[i].deep = 0u;
        CHECK(material_rules_check(&q) == 3);
        q = ok;
        q.bands[i].under_depth = 16u;
        CHECK(material_rules_check(&q) == 3);
        q.bands[i].under_depth = 15u;
        CHECK(material_rules_check(&q) == 0);
        q = ok;
        q.bands[i].y_from = i == 0 ? INT32_MIN + 1 : ok.bands[i - 1].y_from;  // the first not INT32_MIN; a later one not ascending
        CHECK(material_rules_check(&q) == 3);
        if (i > 0) {
            q.bands[i].y_from = ok.bands[i - 1].y_from - (i > 1 ? 1 : 0);
            CHECK(material_rules_check(&q) == 3);
            q.n_bands = (uint32_t)i;  // the faulty band is now outside the bands in use
            CHECK(material_rules_check(&q) == 0);
        }
    }
    {
        vxrt_material_rules q = ok;
        q.n_bands = 1u;
        q.bands[1].top = 0u;
        q.bands[2].y_from = INT32_MIN;
        CHECK(material_rules_check(&q) == 0);
    }
    // ---- the paint box: the limits of vxrt_light_frame's box ----
    const int32_t dims[][4] = {{1, 1, 1, 1}, {1 << 28, 1, 1, 1}, {1 << 10, 1 << 10, 1 << 8, 1}, {1 << 14, 1, 1 << 14, 1}, {0, 1, 1, 0}, {1, -1, 1, 0},
                               {1, 1, 0, 0}, {(1 << 28) + 1, 1, 1, 0}, {1 << 10, 1 << 10, (1 << 8) + 1, 0}, {INT32_MAX, INT32_MAX, INT32_MAX, 0},
                               {1 << 16, 1 << 16, 1 << 16, 0}, {INT32_MIN, 1, 1, 0}};
    for (const auto& d : dims) {
        vxrt_material_rules q = ok;
        for (int k = 0; k < 3; ++k) {
            q.paint_dims[k] = d[k];
            q.paint_origin[k] = 0;
        }
        CHECK(material_paint_ok(q) == (d[3] != 0));
        // the field's box has the same limits on its dims
        const int32_t o[3] = {0, 0, 0}, dd[3] = {d[0], d[1], d[2]};
        CHECK(material_box_check(o, dd) == (d[3] ? 0 : 1));
    }
    for (int k = 0; k < 3; ++k)
        for (int32_t d : {1, 5, 1 << 20}) {
            vxrt_material_rules q = ok;
            q.paint_dims[0] = q.paint_dims[1] = q.paint_dims[2] = 1;
            q.paint_dims[k] = d;
            q.paint_origin[0] = q.paint_origin[1] = q.paint_origin[2] = INT32_MIN;
            CHECK(material_paint_ok(q));
            q.paint_origin[k] = INT32_MAX - d;
            CHECK(material_paint_ok(q));
            q.paint_origin[k] = INT32_MAX - d + 1;
            CHECK(!material_paint_ok(q));
            // the field's box: origin + dims + 16 <= 2^31 - 1, and the dims are looked at before the origin
            int32_t o[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, dd[3] = {1, 1, 1};
            dd[k] = d;
            CHECK(material_box_check(o, dd) == 0);
            o[k] = INT32_MAX - d - 16;
            CHECK(material_box_check(o, dd) == 0);
            o[k] = INT32_MAX - d - 15;
            CHECK(material_box_check(o, dd) == 2);
            dd[(k + 1) % 3] = 0;
            CHECK(material_box_check(o, dd) == 1);
        }
    // ---- the frame: every later fault in place; mended one by one, in the documented order ----
    vxrt_material_frame_params p = good_params();
    p.struct_size -= 4u;
    p.n_tiles = 4097u;
    p.cam.up[1] = inf;
    r = good_rules();
    r.n_bands = 0u;
    r.paint_dims[2] = 0;
    CHECK(material_frame_check(0u, 8u, &p, &r, true) == 2);
    CHECK(material_frame_check(16u, 8u, nullptr, &r, true) == 3);
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 3);
    p.struct_size = sizeof p;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 4);
    p.n_tiles = 4096u;
    p.tile_shift = 7u;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 4);
    p.tile_shift = 6u;
    p.reserved_ = -1;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 4);
    p.reserved_ = 0;
    CHECK(material_frame_check(16u, 8u, &p, nullptr, true) == 5);
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 6);
    r.n_bands = 2u;
    r.bands[1].deep = 0u;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 7);
    r.bands[1].deep = 9u;
    r.reserved_ = 5;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 8);
    r.reserved_ = 0;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 9);
    for (int k = 0; k < 12; ++k)
        for (float v : {nan, inf, -inf}) {
            vxrt_material_frame_params q = good_params();
            (&q.cam.origin[0])[k] = v;
            CHECK(material_frame_check(16u, 8u, &q, &r, true) == 9);
        }
    p.cam.up[1] = 0.0f;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 10);
    CHECK(material_frame_check(16u, 8u, &p, &r, false) == 0);  // without paint the box is not looked at
    r.paint_dims[2] = 1;
    CHECK(material_frame_check(16u, 8u, &p, &r, true) == 0);
    for (uint32_t s = 0; s <= 6u; ++s) {
        p.tile_shift = s;
        p.n_tiles = s & 1u ? 0u : 4096u;
        CHECK(material_frame_check(16u, 8u, &p, &r, true) == 0);
    }
    const uint32_t frames[][3] = {{1, 1, 1}, {65535, 1, 1}, {1, 65535, 1}, {8192, 8192, 1}, {65535, 1024, 1}, {0, 8, 0}, {8, 0, 0},
                                  {65536, 1, 0}, {1, 65536, 0}, {8193, 8192, 0}, {65535, 1025, 0}};
    for (const auto& fr : frames)
        CHECK(material_frame_check(fr[0], fr[1], &p, &r, true) == (fr[2] != 0u ? 0 : 2));
    // ---- what the field launch takes is what the call gave, cut into tasks that cover the box ----
    alignas(4) static uint8_t buf[8];
    const int32_t boxes[][3] = {{1, 1, 1}, {3, 1, 64}, {4, 64, 1}, {5, 65, 2}, {252, 7, 9}, {253, 128, 3}, {256, 1, 1}, {257, 200, 5}, {1 << 28, 1, 1}, {1, 1 << 28, 1}, {1, 1, 1 << 28}};
    for (const auto& b : boxes)
        for (uint32_t seg : {1u, 7u, 64u, 0x7FFFFFFFu}) {
            MaterialFieldArgs A{};
            const int32_t o[3] = {-7, INT32_MIN, 9}, d[3] = {b[0], b[1], b[2]};
            material_field_args(A, ok, o, d, seg, buf + (b[1] & 1));
            const uint64_t lanes_x = (uint64_t)A.nxc << A.lgL, zpw = 64u >> A.lgL;
            CHECK(A.o[0] == -7 && A.o[1] == INT32_MIN && A.o[2] == 9 && A.d[0] == d[0] && A.d[1] == d[1] && A.d[2] == d[2] && A.seg == seg);
            CHECK(A.lgL <= 6u && 4u * lanes_x >= (uint64_t)d[0] && (A.nxc == 1u ? (A.lgL == 0u || (2u << A.lgL) < (uint64_t)d[0] + 4u) : A.lgL == 6u));
            CHECK((uint64_t)(A.nxc - 1u) * 256u < (uint64_t)d[0] && (uint64_t)A.nys * seg >= (uint64_t)d[1] && (uint64_t)(A.nys - 1u) * seg < (uint64_t)d[1]);
            CHECK((uint64_t)A.nzg * zpw >= (uint64_t)d[2] && (uint64_t)(A.nzg - 1u) * zpw < (uint64_t)d[2]);
            CHECK(A.tasks == (uint64_t)A.nxc * A.nys * A.nzg && A.tasks <= (uint64_t)d[0] * d[1] * d[2]);
            CHECK(A.dword == (d[0] % 4 == 0 && (b[1] & 1) == 0 ? 1u : 0u) && A.out == buf + (b[1] & 1) && A.rules.n_bands == 8u);
        }
    // the segment the call picks: 64 rows where that gives eight waves per SIMD (32 per compute unit), else halved, not below 16
    {
        const int32_t small[3] = {128, 128, 128}, window[3] = {512, 128, 512}, large[3] = {1024, 256, 1024}, flat[3] = {4096, 1, 4096};
        CHECK(material_field_segment(small, 256u) == 16u && material_field_segment(window, 256u) == 16u);
        CHECK(material_field_segment(large, 256u) == 64u && material_field_segment(large, 1u << 20) == 16u);
        CHECK(material_field_segment(window, 32u) == 64u && material_field_segment(window, 64u) == 64u && material_field_segment(window, 65u) == 32u);
        CHECK(material_field_segment(flat, 256u) == 64u && material_field_segment(small, 1u) == 64u && material_field_segment(small, 4u) == 64u &&
              material_field_segment(small, 5u) == 32u);
    }
    printf("%llu cases, failures %d\n%s\n", (unsigned long long)cases, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
