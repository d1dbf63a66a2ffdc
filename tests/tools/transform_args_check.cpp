// Host check of the argument limits of the stamp orientations (voxelengine_amd/csrc/vxrt_transform.hpp: orient_valid,
// transform_plan, transform_overlap, transform_check, transform_groups), compiled for the CPU through tests/tools/hoststub.
// No device and no buffers behind the pointers: the 48 valid orientations and the invalid ones around them, the dims and
// the word caps at the last value accepted and the first refused, overlap at the first and the last shared byte, the order
// of the refusals (an earlier check's failure wins), and the launch plan of the shapes at the limits.  Run by
// tests/test_transform_host.py.
//
//   transform_args_check
//   stdout: cases checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

#include "../../voxelengine_amd/csrc/vxrt_transform.hpp"
#include "hbm_world.h"
using namespace vxrt;

int main()
{
    uint64_t cases = 0;
    // orientations: axis a permutation of {0, 1, 2}, flip below 8
    int valid = 0, rotations = 0;
    for (int a = -1; a <= 3; ++a) for (int b = -1; b <= 3; ++b) for (int c = -1; c <= 3; ++c) for (uint32_t f = 0; f < 10u; ++f) {
        const Orient o{{a, b, c}, f};
        const bool perm = a >= 0 && a <= 2 && b >= 0 && b <= 2 && c >= 0 && c <= 2 && a != b && a != c && b != c;
        CHECK(orient_valid(o) == (perm && f < 8u));
        if (orient_valid(o)) {
            ++valid;
            rotations += orient_is_rotation(o) ? 1 : 0;
        }
        ++cases;
    }
    CHECK(valid == 48 && rotations == 24);
    CHECK(!orient_valid(Orient{{0, 1, 2}, 1u << 31}) && !orient_valid(Orient{{INT32_MIN, 1, 2}, 0u}) && !orient_valid(Orient{{0, 1, INT32_MAX}, 0u}));

    const Orient id{{0, 1, 2}, 0u}, zturn{{1, 0, 2}, 1u}, xz{{2, 1, 0}, 0u};
    TransformArgs A;
    // dims: vxrt_region_words' contract
    const int32_t bad_dims[][3] = {{0, 8, 8}, {8, -1, 8}, {8, 8, 0}, {INT32_MIN, 1, 1}, {1 << 20, 1 << 16, 2}, {INT32_MAX, INT32_MAX, 1}};
    for (const auto& d : bad_dims) {
        CHECK(transform_plan(d, id, A) == 1 && transform_plan(d, zturn, A) == 1);
        ++cases;
    }
    // the word caps.  A row of one voxel still takes a word: (1, 2^16, 2^15) is 2^31 voxels in 2^31 words, the last shape
    // accepted; (1, 2^16, 2^15 + 1) passes the cap with few voxels.
    {
        const int32_t at[3] = {1, 1 << 16, 1 << 15}, over[3] = {1, 1 << 16, (1 << 15) + 1}, limit[3] = {1, 1 << 15, (1 << 15) + 1};
        CHECK(region_words(at) == kTransformMaxWords && region_words(over) > kTransformMaxWords && region_words(over) != 0);
        CHECK(transform_plan(at, id, A) == 0 && A.nsrc == kTransformMaxWords && A.ndst == kTransformMaxWords);
        CHECK(transform_plan(over, id, A) == 2 && transform_plan(over, zturn, A) == 2 && transform_plan(over, xz, A) == 2);
        // the GPU suite's limit case: more than 2^32 bytes of source in about 2^30 voxels
        CHECK(transform_plan(limit, id, A) == 0 && 4u * A.nsrc > (1ull << 32) && A.nsrc == (1ull << 30) + (1u << 15));
        CHECK(transform_plan(limit, zturn, A) == 0 && A.dd[0] == 1 << 15 && A.dd[1] == 1 && A.ndst == 1024ull * ((1u << 15) + 1u));
        CHECK(A.tiles == (uint64_t)(1024u / kTrTJ) * ((1u << 15) + 1u) && transform_groups(A) == kTrMaxGroups);
        // the destination alone beyond the cap: 32-voxel rows become 32 rows of one voxel
        const int32_t wide[3] = {32, 1, INT32_MAX};
        CHECK(region_words(wide) == (uint64_t)INT32_MAX);
        CHECK(transform_plan(wide, id, A) == 0 && transform_plan(wide, zturn, A) == 2);
        // and the source alone: the inverse direction
        const int32_t tall[3] = {1, 32, INT32_MAX};
        CHECK(region_words(tall) == 32ull * INT32_MAX && transform_plan(tall, zturn, A) == 2 && transform_plan(tall, id, A) == 2);
        const int32_t row[3] = {INT32_MAX, 1, 32};  // 2^26 words a row
        CHECK(transform_plan(row, id, A) == 0 && A.wps == 1u << 26 && A.nsrc == 1ull << 31);
        CHECK(transform_plan(row, xz, A) == 0 && A.wpd == 1u && A.ndst == 32ull * INT32_MAX / 32u && A.tiles == (uint64_t)((1u << 26) / kTrTX));
        cases += 12;
    }
    // the plan of every orientation on a small box: dims, classes, tiles
    {
        const int32_t sd[3] = {33, 70, 5};
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) for (int c = 0; c < 3; ++c) for (uint32_t f = 0; f < 8u; ++f) {
            const Orient o{{a, b, c}, f};
            if (!orient_valid(o))
                continue;
            CHECK(transform_plan(sd, o, A) == 0);
            CHECK(A.dd[0] == sd[a] && A.dd[1] == sd[b] && A.dd[2] == sd[c] && A.nsrc == 2u * 70u * 5u && A.ndst == region_words(A.dd));
            if (a != 0) {
                CHECK(A.s == a && A.t == 3 - a && A.axis[A.kx] == 0 && A.axis[A.kt] == A.t);
                CHECK(A.tiles_x == 1u && A.tiles_j == (A.wpd + kTrTJ - 1u) / kTrTJ && A.tiles == (uint64_t)A.tiles_j * (uint64_t)sd[A.t]);
                CHECK(transform_groups(A) == A.tiles);
            } else {
                CHECK(transform_groups(A) == (A.ndst + kTrLanes - 1u) / kTrLanes);
            }
            ++cases;
        }
    }
    // overlap: byte ranges, at the first and the last byte shared
    {
        char* const base = (char*)(uintptr_t)0x10000000u;
        CHECK(transform_overlap(base, 64, base, 64) && transform_overlap(base, 64, base + 63, 4) && transform_overlap(base + 63, 4, base, 64));
        CHECK(!transform_overlap(base, 64, base + 64, 64) && !transform_overlap(base + 64, 64, base, 64));
        CHECK(transform_overlap(base, 1024, base + 512, 4) && transform_overlap(base + 512, 4, base, 1024));
        char* const high = (char*)(uintptr_t)0x7FFF00000000ull;  // ranges of more than 2^32 bytes
        CHECK(transform_overlap(high, 5ull << 30, high + (5ull << 30) - 1, 8) && !transform_overlap(high, 5ull << 30, high + (5ull << 30), 8));
        cases += 8;
    }
    // the order of the refusals: NULL arguments, the orientation, the dims, the caps, overlap
    {
        uint32_t* const p = (uint32_t*)(uintptr_t)0x10000000u;
        const int32_t good[3] = {33, 4, 4}, nodims[3] = {0, 4, 4}, over[3] = {1, 1 << 16, (1 << 15) + 1};
        const Orient bad{{0, 0, 2}, 9u}, badflip{{0, 1, 2}, 8u};
        const uint64_t n = region_words(good);
        CHECK(transform_check(p, good, &zturn, p + n, A) == 0 && A.src == p && A.dst == p + n && A.summary == nullptr);
        CHECK(transform_check(p + n, good, &zturn, p, A) == 5);  // (the turned stamp is 132 words: it reaches the source)
        CHECK(transform_check(nullptr, nodims, &bad, p, A) == 1 && transform_check(p, nullptr, &bad, p, A) == 1);
        CHECK(transform_check(p, nodims, nullptr, p, A) == 1 && transform_check(p, nodims, &bad, nullptr, A) == 1);
        CHECK(transform_check(p, nodims, &bad, p, A) == 2 && transform_check(p, over, &badflip, p, A) == 2);
        CHECK(transform_check(p, nodims, &zturn, p, A) == 3);
        CHECK(transform_check(p, over, &zturn, p, A) == 4);
        CHECK(transform_check(p, good, &zturn, p, A) == 5 && transform_check(p, good, &zturn, p + n - 1, A) == 5);
        // (the destination of the turn is 4 x 33 x 4: one word a row, 132 words)
        CHECK(transform_check(p + 132u - 1u, good, &zturn, p, A) == 5 && transform_check(p + 132u, good, &zturn, p, A) == 0);
        cases += 14;
    }
    // the division by a launch's fixed divisor, exact for every numerator below 2^31
    {
        uint32_t lcg = 99u;
        const uint32_t ds[] = {1u, 2u, 3u, 5u, 7u, 8u, 9u, 31u, 32u, 33u, 1000u, 1023u, 1024u, 1025u, 65535u, 65536u, 65537u, 1u << 26,
                               (1u << 30) - 1u, 1u << 30, (1u << 30) + 1u, 0x7FFFFFFEu, 0x7FFFFFFFu};
        for (uint32_t d : ds) {
            const TrDiv f = tr_div_by(d);
            for (uint64_t k = 0; k < 40u; ++k)  // around the multiples of d, and the ends
                for (int64_t e = -2; e <= 2; ++e) {
                    const int64_t n = (int64_t)((k * 0x7FFFFFFFull / 39u) / d * d) + e;
                    if (n >= 0 && n <= 0x7FFFFFFF)
                        CHECK(tr_div((uint32_t)n, f) == (uint32_t)n / d);
                }
            for (int i = 0; i < 2000; ++i) {
                const uint32_t n = (lcg = lcg * 1664525u + 1013904223u) >> 1;
                CHECK(tr_div(n, f) == n / d);
            }
            CHECK(tr_div(0x7FFFFFFFu, f) == 0x7FFFFFFFu / d && tr_div(0u, f) == 0u && tr_div(d - 1u, f) == 0u && tr_div(d, f) == 1u);
            ++cases;
        }
        for (uint32_t d = 1; d < 3000u; ++d) {
            const TrDiv f = tr_div_by(d);
            for (uint32_t n : {0x7FFFFFFFu, 0x7FFFFFFFu / d * d, 0x7FFFFFFFu / d * d - 1u, 123456789u})
                CHECK(tr_div(n, f) == n / d);
        }
    }
    // the rotation helper: one turn about z is {1, 0, 2} with flip 1; four turns are the identity; negative and large counts
    {
        Orient r;
        CHECK(orient_rotation(2, 1, r) && r.axis[0] == 1 && r.axis[1] == 0 && r.axis[2] == 2 && r.flip == 1u);
        for (int axis = 0; axis < 3; ++axis)
            for (int n : {-9, -4, -1, 0, 3, 4, 5, 1 << 30, INT32_MIN, INT32_MAX}) {
                Orient want = id, q;
                CHECK(orient_rotation(axis, 1, q));
                for (int i = 0; i < (((n % 4) + 4) % 4); ++i)
                    want = orient_compose(want, q);
                CHECK(orient_rotation(axis, n, r) && r.axis[0] == want.axis[0] && r.axis[1] == want.axis[1] && r.axis[2] == want.axis[2] && r.flip == want.flip);
                CHECK(orient_is_rotation(r));
                ++cases;
            }
        CHECK(!orient_rotation(-1, 1, r) && !orient_rotation(3, 1, r));
    }
    printf("%llu cases, failures %d\n%s\n", (unsigned long long)cases, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
