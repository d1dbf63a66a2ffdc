// Host check of the argument limits of the neighbour-count voxel rules (voxelengine_amd/csrc/vxrt_rule.hpp: rule_check,
// rule_halo, rule_layout) and of the two word helpers every lane leans on (rule_span, rule_gather), compiled for the CPU
// through tests/tools/hoststub.  No world and no device: the limits of the rule's fields in the documented order, of dims,
// the halo box and the origin at the first value refused and the last accepted, the workspace formula of include/vxrt.h,
// and the helpers against bit-by-bit loops.  Run by tests/test_rule_host.py.
//
//   rule_args_check
//   stdout: cases checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_RULE_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_rule.hpp"
#include "hbm_world.h"
#include <vector>
using namespace vxrt;

static vxrt_rule rule_of(int32_t nb, uint32_t born, uint32_t survive, int32_t it, int32_t scope, int32_t outside)
{
    vxrt_rule r{};
    r.struct_size = sizeof(vxrt_rule);
    r.neighbours = nb;
    r.born = born;
    r.survive = survive;
    r.iterations = it;
    r.scope = scope;
    r.outside = outside;
    return r;
}

static uint64_t up256(uint64_t n) { return (n + 255u) / 256u * 256u; }

int main()
{
    uint64_t cases = 0;
    // the rule's fields, each alone and in the documented order (an earlier field's failure wins)
    const vxrt_rule good = rule_of(kRuleN26, 1u << 26, 1u, 16, kRuleWorld, 1);
    CHECK(rule_check(good) == 0 && rule_halo(good) == 16);
    CHECK(rule_halo(rule_of(kRuleN6, 0u, 0u, 16, kRuleBox, 0)) == 1);
    {
        vxrt_rule r = good;
        r.struct_size -= 4u;
        r.neighbours = 7;
        CHECK(rule_check(r) == 1);
        r = good;
        r.neighbours = 3;
        r.born = ~0u;
        CHECK(rule_check(r) == 2);
        r.neighbours = -1;
        CHECK(rule_check(r) == 2);
        const uint32_t n_of[3] = {6u, 18u, 26u};
        for (int nb = 0; nb < 3; ++nb) {
            CHECK(rule_neighbours(nb) == n_of[nb]);
            const uint32_t all = (2u << n_of[nb]) - 1u;
            CHECK(rule_check(rule_of(nb, all, all, 1, kRuleBox, 0)) == 0);
            CHECK(rule_check(rule_of(nb, all + 1u, 0u, 1, kRuleBox, 0)) == 3);
            CHECK(rule_check(rule_of(nb, 0u, all + 1u, 0, kRuleBox, 0)) == 3);
            CHECK(rule_check(rule_of(nb, 0u, 1u << 31, 1, kRuleBox, 0)) == 3);
            cases += 4;
        }
        for (int32_t it : {0, -1, 17, INT32_MAX, INT32_MIN})
            CHECK(rule_check(rule_of(kRuleN6, 1u, 1u, it, 2, 0)) == 4);
        CHECK(rule_check(rule_of(kRuleN6, 1u, 1u, 1, kRuleBox, 0)) == 0 && rule_check(rule_of(kRuleN6, 1u, 1u, 16, kRuleBox, 0)) == 0);
        for (int32_t scope : {-1, 2, INT32_MAX})
            CHECK(rule_check(rule_of(kRuleN6, 1u, 1u, 1, scope, 2)) == 5);
        for (int32_t outside : {-1, 2, INT32_MIN})
            CHECK(rule_check(rule_of(kRuleN6, 1u, 1u, 1, kRuleBox, outside)) == 6);
        r = good;
        r.reserved_ = 1;
        CHECK(rule_check(r) == 7);
        cases += 16;
    }

    // dims: each at least 1, the product at most 2^28, the halo box at most 2^36 voxels
    RuleLayout L{};
    const int32_t zero[3] = {0, 0, 0};
    for (int32_t h : {1, 16}) {
        const int32_t bad[][3] = {{0, 8, 8}, {8, -1, 8}, {8, 8, 0}, {1 << 10, 1 << 10, (1 << 8) + 1}, {1 << 29, 1, 1}, {INT32_MAX, 1, 1}};
        for (const auto& d : bad) {
            CHECK(!rule_layout(nullptr, d, h, L) && !rule_layout(zero, d, h, L));
            ++cases;
        }
        // ((2^28, 1, 1): a halo of (2^28 + 2) x 3 x 3 voxels at h = 1, of (2^28 + 32) x 33 x 33 > 2^36 at h = 16)
        const int32_t ok[][3] = {{1, 1, 1}, {1 << 10, 1 << 10, 1 << 8}, {1 << 14, 1 << 14, 1}, {1 << 28, 1, 1}};
        for (const auto& d : ok) {
            if (d[0] == 1 << 28 && h == 16) {
                CHECK(!rule_layout(nullptr, d, h, L));
                continue;
            }
            CHECK(rule_layout(nullptr, d, h, L) && rule_layout(zero, d, h, L));
            const uint64_t hd[3] = {(uint64_t)d[0] + 2u * h, (uint64_t)d[1] + 2u * h, (uint64_t)d[2] + 2u * h};
            CHECK(L.total_bytes == 4u * up256(4u * ((hd[0] + 31u) / 32u) * hd[1] * hd[2]));
            CHECK(L.wh == (hd[0] + 31u) / 32u && L.hy == hd[1] && L.hz == hd[2] && L.mw == ((uint64_t)d[0] + 31u) / 32u && L.h == (uint32_t)h);
            CHECK(L.np == (uint64_t)L.wh * L.hy * L.hz && L.nb == (uint64_t)L.mw * d[1] * d[2]);
            ++cases;
        }
    }
    // the halo box against 2^36 voxels: (1, 1, 2^28) has a halo of 3 x 3 x (2^28 + 2) < 2^36 at h = 1 and of
    // 33 x 33 x (2^28 + 32) > 2^36 at h = 16; h = 3 gives 49 x (2^28 + 6) < 2^36, h = 8 gives 289 x (2^28 + 16) > 2^36
    {
        const int32_t d[3] = {1, 1, 1 << 28};
        CHECK(rule_layout(nullptr, d, 1, L) && rule_layout(nullptr, d, 3, L) && !rule_layout(nullptr, d, 8, L) && !rule_layout(nullptr, d, 16, L));
        CHECK(!rule_layout(nullptr, d, 0, L) && !rule_layout(nullptr, d, 17, L));
        cases += 6;
    }
    // the origin: origin - h >= -2^31 and origin + dims + h <= 2^31 - 1, at the last value accepted and the first refused
    for (int32_t h : {1, 2, 16}) {
        const int32_t dims[2][3] = {{8, 8, 8}, {1, 3, 70}};
        for (const auto& d : dims)
            for (int k = 0; k < 3; ++k) {
                const int64_t lo = (int64_t)INT32_MIN + h, hi = (int64_t)INT32_MAX - d[k] - h;
                const int64_t edge[4] = {lo, lo - 1, hi, hi + 1};
                for (int e = 0; e < 4; ++e) {
                    int32_t o[3] = {0, 0, 0};
                    o[k] = (int32_t)edge[e];
                    CHECK(rule_layout(o, d, h, L) == (e % 2 == 0));
                    CHECK(rule_layout(nullptr, d, h, L));
                    ++cases;
                }
            }
    }

    // rule_span against a loop, at word starts around both ends of the range and at the ends of int32
    const int64_t starts[] = {-70, -33, -32, -31, -1, 0, 1, 30, 31, 32, 33, 63, 64, 100, (int64_t)INT32_MIN - 16, (int64_t)INT32_MAX - 20};
    const int64_t ranges[][2] = {{0, 63}, {0, 0}, {5, 4}, {31, 32}, {-40, -35}, {0, 31}, {INT32_MIN, INT32_MAX}, {INT32_MAX, INT32_MAX}};
    for (int64_t x0 : starts)
        for (const auto& r : ranges) {
            uint32_t want = 0u;
            for (int j = 0; j < 32; ++j)
                if (x0 + j >= r[0] && x0 + j <= r[1])
                    want |= 1u << j;
            CHECK(rule_span(x0, r[0], r[1]) == want);
            ++cases;
        }
    // rule_gather against a loop: bit sx + j of a row of nw words, 0 outside the row; every index within the array
    uint32_t lcg = 12345u;
    for (uint64_t nw : {1u, 2u, 3u}) {
        std::vector<uint32_t> rows(3u * nw);
        for (uint32_t& v : rows)
            v = (lcg = lcg * 1664525u + 1013904223u);
        g_size[kRulePlane] = rows.size();
        for (uint64_t row = 0; row < 3u; ++row)
            for (int64_t sx = -40; sx <= 32 * (int64_t)nw + 8; ++sx) {
                uint32_t want = 0u;
                for (int j = 0; j < 32; ++j) {
                    const int64_t x = sx + j;
                    if (x >= 0 && x < 32 * (int64_t)nw && ((rows[row * nw + (uint64_t)(x >> 5)] >> (x & 31)) & 1u))
                        want |= 1u << j;
                }
                CHECK(rule_gather(kRulePlane, rows.data(), row * nw, nw, sx) == want);
                ++cases;
            }
    }
    printf("%llu cases, %llu indices checked, failures %d\n%s\n", (unsigned long long)cases, (unsigned long long)checked, fails,
           fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
