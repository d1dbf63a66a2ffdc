// Host check of the argument limits of the loose voxels (voxelengine_amd/csrc/vxrt_loose.hpp: loose_check, loose_layout and
// the pass schedule) and of the two word helpers every lane leans on (loose_span, loose_gather), compiled for the CPU through
// tests/tools/hoststub.  No world and no device: the limits of the parameters' fields in the documented order, of dims, the
// halo box and the origin at the first value refused and the last accepted, the workspace formula of include/vxrt.h, the
// planes and step numbers of the passes, and the helpers against bit-by-bit loops.  Run by tests/test_loose_host.py.
//
//   loose_args_check
//   stdout: cases checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_LOOSE_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_loose.hpp"
#include "hbm_world.h"
#include <vector>
using namespace vxrt;

static vxrt_loose params_of(int32_t material, int32_t steps, int32_t edge, uint32_t phase)
{
    vxrt_loose q{};
    q.struct_size = sizeof(vxrt_loose);
    q.material = material;
    q.steps = steps;
    q.edge = edge;
    q.phase = phase;
    return q;
}

static uint64_t up256(uint64_t n) { return (n + 255u) / 256u * 256u; }

int main()
{
    uint64_t cases = 0;
    // the fields, each alone and in the documented order (an earlier field's failure wins)
    const vxrt_loose good = params_of(kLooseWater, 64, kLooseOpen, 0xFFFFFFFFu);
    CHECK(loose_check(good) == 0 && loose_check(params_of(kLooseSand, 1, kLooseWall, 0u)) == 0);
    {
        vxrt_loose q = good;
        q.struct_size -= 4u;
        q.material = 7;
        CHECK(loose_check(q) == 1);
        for (int32_t m : {-1, 2, INT32_MAX, INT32_MIN}) {
            q = params_of(m, 0, 5, 0u);
            q.reserved_[1] = 1;
            CHECK(loose_check(q) == 2);
        }
        for (int32_t s : {0, -1, 65, INT32_MAX, INT32_MIN}) {
            q = params_of(kLooseSand, s, 5, 0u);
            q.reserved_[0] = 1;
            CHECK(loose_check(q) == 3);
        }
        for (int32_t e : {-1, 2, INT32_MAX}) {
            q = params_of(kLooseSand, 1, e, 0u);
            q.reserved_[2] = 1;
            CHECK(loose_check(q) == 4);
        }
        for (int k = 0; k < 3; ++k) {
            q = good;
            q.reserved_[k] = k == 1 ? -1 : 1;
            CHECK(loose_check(q) == 5);
        }
        cases += 16;
    }
    // the schedule: sand FALL, SLIDE; water FALL, SLIDE, SPREAD; step numbers from `phase`, wrapping; the planes in turn
    {
        LooseArgs A{};
        uint32_t a, b;
        A.turn[0] = &a;
        A.turn[1] = &b;
        const vxrt_loose sand = params_of(kLooseSand, 3, kLooseWall, 0xFFFFFFFEu), water = params_of(kLooseWater, 64, kLooseWall, 5u);
        CHECK(loose_passes(sand) == 6 && loose_passes(water) == 192);
        const int sk[6] = {kLooseFall, kLooseSlide, kLooseFall, kLooseSlide, kLooseFall, kLooseSlide};
        const uint32_t st[6] = {0xFFFFFFFEu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
        for (int p = 0; p < 6; ++p) {
            CHECK(loose_pass_kind(kLooseSand, p) == sk[p] && loose_pass_step(sand, p) == st[p]);
            CHECK(loose_src(A, p) == (p & 1 ? &b : &a) && loose_dst(A, p) == (p & 1 ? &a : &b));
        }
        for (int p = 0; p < 192; ++p)
            CHECK(loose_pass_kind(kLooseWater, p) == p % 3 && loose_pass_step(water, p) == 5u + (uint32_t)(p / 3));
        CHECK(loose_src(A, 192) == &a && loose_src(A, 6) == &a && loose_src(A, 3) == &b);
        cases += 200;
    }

    // dims: each at least 1, the product at most 2^28, the halo box at most 2^36 voxels
    LooseLayout L{};
    const int32_t zero[3] = {0, 0, 0};
    const int32_t bad[][3] = {{0, 8, 8}, {8, -1, 8}, {8, 8, 0}, {1 << 10, 1 << 10, (1 << 8) + 1}, {1 << 29, 1, 1}, {INT32_MAX, 1, 1}};
    for (const auto& d : bad) {
        CHECK(!loose_layout(nullptr, d, L) && !loose_layout(zero, d, L) && L.fault == kBoxDims);
        ++cases;
    }
    const int32_t ok[][3] = {{1, 1, 1}, {31, 2, 3}, {1 << 10, 1 << 10, 1 << 8}, {1 << 14, 1, 1 << 14}, {1 << 28, 1, 1}, {1, 1, 1 << 28}, {1, 1 << 28, 1}};
    for (const auto& d : ok) {
        CHECK(loose_layout(nullptr, d, L) && loose_layout(zero, d, L));
        const uint64_t hd[3] = {(uint64_t)d[0] + 2u, (uint64_t)d[1] + 2u, (uint64_t)d[2] + 2u};
        CHECK(L.total_bytes == 4u * up256(4u * ((hd[0] + 31u) / 32u) * hd[1] * hd[2]));
        CHECK(L.wh == (hd[0] + 31u) / 32u && L.hy == hd[1] && L.hz == hd[2] && L.mw == ((uint64_t)d[0] + 31u) / 32u);
        CHECK(L.np == (uint64_t)L.wh * L.hy * L.hz && L.nb == (uint64_t)L.mw * d[1] * d[2]);
        CHECK(L.ho[0] == -1 && L.ho[1] == -1 && L.ho[2] == -1 && L.hd[0] == d[0] + 2 && L.hd[1] == d[1] + 2 && L.hd[2] == d[2] + 2);
        ++cases;
    }
    // the origin: origin - 1 >= -2^31 and origin + dims + 1 <= 2^31 - 1, at the last value accepted and the first refused
    {
        const int32_t dims[2][3] = {{8, 8, 8}, {1, 3, 70}};
        for (const auto& d : dims)
            for (int k = 0; k < 3; ++k) {
                const int64_t lo = (int64_t)INT32_MIN + 1, hi = (int64_t)INT32_MAX - d[k] - 1;
                const int64_t edge[4] = {lo, lo - 1, hi, hi + 1};
                for (int e = 0; e < 4; ++e) {
                    int32_t o[3] = {0, 0, 0};
                    o[k] = (int32_t)edge[e];
                    CHECK(loose_layout(o, d, L) == (e % 2 == 0));
                    CHECK(e % 2 == 0 || L.fault == kBoxOrigin);
                    CHECK(loose_layout(nullptr, d, L));
                    ++cases;
                }
            }
    }

    // loose_span against a loop, at word starts around both ends of the range and at the ends of int32
    const int64_t starts[] = {-70, -33, -32, -31, -1, 0, 1, 30, 31, 32, 33, 63, 64, 100, (int64_t)INT32_MIN - 16, (int64_t)INT32_MAX - 20};
    const int64_t ranges[][2] = {{0, 63}, {0, 0}, {5, 4}, {31, 32}, {-40, -35}, {0, 31}, {INT32_MIN, INT32_MAX}, {INT32_MAX, INT32_MAX}};
    for (int64_t x0 : starts)
        for (const auto& r : ranges) {
            uint32_t want = 0u;
            for (int j = 0; j < 32; ++j)
                if (x0 + j >= r[0] && x0 + j <= r[1])
                    want |= 1u << j;
            CHECK(loose_span(x0, r[0], r[1]) == want);
            ++cases;
        }
    // loose_gather against a loop: bit sx + j of a row of nw words, 0 outside the row; every index within the array
    uint32_t lcg = 12345u;
    for (uint64_t nw : {1u, 2u, 3u}) {
        std::vector<uint32_t> rows(3u * nw);
        for (uint32_t& v : rows)
            v = (lcg = lcg * 1664525u + 1013904223u);
        g_size[kLoosePlane] = rows.size();
        for (uint64_t row = 0; row < 3u; ++row)
            for (int64_t sx = -40; sx <= 32 * (int64_t)nw + 8; ++sx) {
                uint32_t want = 0u;
                for (int j = 0; j < 32; ++j) {
                    const int64_t x = sx + j;
                    if (x >= 0 && x < 32 * (int64_t)nw && ((rows[row * nw + (uint64_t)(x >> 5)] >> (x & 31)) & 1u))
                        want |= 1u << j;
                }
                CHECK(loose_gather(kLoosePlane, rows.data(), row * nw, nw, sx) == want);
                ++cases;
            }
    }
    printf("%llu cases, %llu indices checked, failures %d\n%s\n", (unsigned long long)cases, (unsigned long long)checked, fails,
           fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
