// Host check of the output's store width (voxelengine_amd/csrc/vxrt_light.hpp: light_args sets LightArgs::wide from the
// address of d_levels, light_expand_lane stores dwords or bytes by it), compiled for the CPU through tests/tools/hoststub.
// For boxes whose voxel counts are 0, 1, 2 and 3 mod 4 and an output at byte offsets 0 .. 3 of an aligned buffer: light_args
// must clear `wide` exactly off the dword grid, and the expansion of a workspace of pseudo-random planes must give the
// aligned output's bytes at every offset, 0x5A guard bytes before and behind untouched, every index inside its array.
// Run by tests/test_field_limits_host.py.
//
//   light_args_check
//   stdout: lanes expanded, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_LIGHT_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_light.hpp"
#include "hbm_world.h"
#include <vector>
using namespace vxrt;

int main()
{
    const int32_t boxes[5][3] = {{5, 4, 3}, {5, 3, 3}, {7, 3, 2}, {3, 3, 3}, {37, 5, 3}};
    const int32_t o[3] = {0, 0, 0};
    const size_t guard = 16;
    uint64_t lanes = 0;
    for (const auto& d : boxes) {
        for (uint32_t channels = 1; channels <= 3; ++channels) {
            LightLayout L{};
            CHECK(light_layout(o, d, channels, L));
            std::vector<uint32_t> work(L.total_bytes / 4u + 1u);
            uint32_t r = 12345u + channels;
            for (uint32_t& w : work)
                w = (r = r * 1664525u + 1013904223u);
            g_size[kLightPlane] = L.np;
            g_size[kLightOut] = L.nvox;
            uint32_t summary[kLightSumWords] = {};
            std::vector<uint8_t> first;
            for (size_t off = 0; off < 4; ++off) {
                std::vector<uint8_t> buf(guard + L.nvox + guard, 0x5A);
                CHECK(((uintptr_t)buf.data() & 3u) == 0u);
                LightArgs A{};
                light_args(A, L, o, d, channels, work.data(), nullptr, 0u, buf.data() + guard + off, summary);
                CHECK(A.wide == (off == 0 ? 1u : 0u));
                const uint64_t ne = ((uint64_t)L.nvox + 3u) / 4u;
                for (uint64_t j = 0; j < ne; ++j)
                    light_expand_lane(A, j);
                lanes += ne;
                for (size_t i = 0; i < guard + off; ++i)
                    CHECK(buf[i] == 0x5A);
                for (size_t i = guard + off + L.nvox; i < buf.size(); ++i)
                    CHECK(buf[i] == 0x5A);
                const std::vector<uint8_t> got(buf.begin() + (long)(guard + off), buf.begin() + (long)(guard + off + L.nvox));
                if (off == 0) {
                    first = got;
                    bool seen[256] = {};  // the planes are noise: the bytes are not all alike
                    int distinct = 0;
                    for (uint8_t v : got)
                        if (!seen[v]) {
                            seen[v] = true;
                            ++distinct;
                        }
                    CHECK(distinct > 4);
                } else {
                    CHECK(got == first);
                }
            }
        }
    }
    printf("%llu lanes expanded, %llu indices checked, failures %d\n%s\n", (unsigned long long)lanes, (unsigned long long)checked, fails,
           fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
