// Host harness of the occupancy LOD (voxelengine_amd/csrc/vxrt_lod.hpp: the limits and the layout, the lane mapping, the
// bit-parallel field sums, a lane's walk over its source rows, its counts, bits and tallies, the store of an output word),
// compiled for the CPU through tests/tools/hoststub and run one lane at a time, wave by wave in the tasks each takes in turn.  The harness
// restates what k_lod_reduce of vxrt_lod.hip adds around that code, which the GPU suite covers:
//   the SPLIT kernel's LDS add   the four waves' accumulators over a quarter of the cell's z slices each, added word by
//                                word (split = 1 in the header; taken for shift >= 3, where the kernel exists);
//   the xor shuffles             the OR of the words of the lod_group(A) aligned lanes of a wave that hold one output word;
//   the summary                  the lanes' tallies summed (the maximum for max_count) into vxrt_lod_summary's eight words.
// The world is the oracle's brickmap (oracle/vxo_world.c) of a dense grid, laid out as the library holds it in HBM; the
// source box's bits come from region_row_word, clipped as k_read_region clips.  Every index the code forms into the
// workspace or an output is checked against that array's size; the outputs carry a guard behind them.  Run by
// tests/test_lod_host.py, which compares the outputs with tests/ref_lod.py.
//
//   lod_check in.bin out.bin
//   in:  i32 op, f, X, Y, Z, origin[3], dims[3], shift, threshold, counts, split; X * Y * Z / 32 u32 dense words
//   op 0 (downsample): out: 8 u32 summary, region_words(dims) u32 bits, then (counts) dims[0] * dims[1] * dims[2] u16
//   op 1 (limits and layout only; no world is built): out: u32 accepted by lod_layout with the origin, u32 accepted without
//        it, u32 accepted by lod_threshold_ok, u32 0, u64 total_bytes
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_LOD_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_lod.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <vector>
using namespace vxrt;

template <uint32_t SH>
static void run(const LodArgs& A, const LodLayout& L, bool split, uint32_t* summary)
{
    constexpr uint32_t f = 1u << SH;
    const uint32_t group = lod_group(A);
    uint64_t solid = 0;
    std::vector<uint8_t> stored((size_t)A.wpo * A.rows, 0);
    CHECK(group >= 1u && group <= 64u && 64u % group == 0u);
    const uint32_t iters = split ? 1u : A.iters, waves = (L.tasks + iters - 1u) / iters + 3u;  // the last workgroup's idle waves included
    std::vector<uint8_t> taken(L.tasks, 0);
    for (uint32_t wv = 0; wv < waves; ++wv) for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t task = lod_wave_task(wv, iters, it);
        if (task < L.tasks)
            taken[task]++;
        uint32_t word[64], k[64], row[64];
        bool live[64];
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            word[lane] = 0u;
            live[lane] = lod_lane(A, task, lane, k[lane], row[lane]);
            if (!live[lane])
                continue;
            CHECK(task < L.tasks);
            const uint32_t Y = row[lane] % (uint32_t)A.d[1], Z = row[lane] / (uint32_t)A.d[1];
            uint32_t lo = 0u, hi = 0u;
            if (split) {
                for (uint32_t wave = 0; wave < 4u; ++wave) {  // the LDS add, restated
                    uint32_t plo = 0u, phi = 0u;
                    lod_accumulate<SH>(A, k[lane], Y, Z, wave * (f / 4u), (wave + 1u) * (f / 4u), plo, phi);
                    lo += plo;
                    hi += phi;
                }
            } else {
                lod_accumulate<SH>(A, k[lane], Y, Z, 0u, f, lo, hi);
            }
            LodTally t{};
            word[lane] = lod_finish<SH>(A, k[lane], row[lane], lo, hi, t);
            solid += t.solid;
            summary[2] += t.set;
            summary[3] += t.empty;
            summary[4] += t.full;
            summary[5] += t.mixed;
            summary[6] = t.max_count > summary[6] ? t.max_count : summary[6];
        }
        for (uint32_t g = 0; g < 64u; g += group) {  // the xor shuffles, restated: every lane of a group ends with the OR
            uint32_t all = 0u;
            for (uint32_t i = 0; i < group; ++i)
                all |= word[g + i];
            for (uint32_t i = 0; i < group; ++i)
                if (live[g + i]) {
                    if (!(k[g + i] & (f - 1u)))
                        stored[(size_t)row[g + i] * A.wpo + (k[g + i] >> SH)]++;
                    lod_store(A, k[g + i], row[g + i], all);
                    CHECK(row[g + i] == row[g] && (k[g + i] >> SH) == (k[g] >> SH));  // a group holds one output word
                }
        }
    }
    for (size_t i = 0; i < stored.size(); ++i)
        CHECK(stored[i] == 1);  // every output word has exactly one storing lane
    for (size_t i = 0; i < taken.size(); ++i)
        CHECK(taken[i] == 1);  // every task has exactly one wave
    summary[0] = (uint32_t)solid;
    summary[1] = (uint32_t)(solid >> 32);
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: lod_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[15];
    if (!in || fread(hd, 4, 15, in) != 15)
        return 2;
    const int op = hd[0], f = hd[1], X = hd[2], Y = hd[3], Z = hd[4];
    const int32_t o[3] = {hd[5], hd[6], hd[7]}, d[3] = {hd[8], hd[9], hd[10]};
    const uint32_t shift = (uint32_t)hd[11], threshold = (uint32_t)hd[12], counts = (uint32_t)hd[13];
    const bool split = hd[14] != 0 && shift >= 3u;
    LodLayout L{};
    if (op == 1) {
        fclose(in);
        const uint32_t with = lod_layout(o, d, shift, L) ? 1u : 0u, without = lod_layout(nullptr, d, shift, L) ? 1u : 0u;
        const uint64_t bytes = without ? L.total_bytes : 0u;
        FILE* out = fopen(argv[2], "wb");
        if (!out)
            return 2;
        fwrite(&with, 4, 1, out);
        fwrite(&without, 4, 1, out);
        const uint32_t thr[2] = {lod_threshold_ok(shift, threshold) ? 1u : 0u, 0u};
        fwrite(thr, 4, 2, out);
        fwrite(&bytes, 8, 1, out);
        fclose(out);
        printf("layout %u %u\nALL OK\n", with, without);
        return 0;
    }
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    if (fread(dense.data(), 4, dense.size(), in) != dense.size())
        return 2;
    fclose(in);

    // the oracle's brickmap in HBM order
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    const HbmWorld h = to_hbm(w);
    vxo_world_free(w);

    if (!lod_layout(o, d, shift, L) || !lod_threshold_ok(shift, threshold)) {
        printf("outside the contract\n");
        return 2;
    }
    const uint32_t guard = 0x5A5A5A5Au;
    const uint64_t nbits = region_words(d), ncells = (uint64_t)d[0] * d[1] * d[2];
    std::vector<uint8_t> work(L.total_bytes, 0xA5);
    std::vector<uint32_t> bits(nbits + 1u, guard);
    std::vector<uint16_t> cnt(ncells + 1u, (uint16_t)guard);
    uint32_t summary[8] = {};
    g_size[kLodSrc] = L.nsrc;
    g_size[kLodBits] = nbits;
    g_size[kLodCounts] = counts ? ncells : 0u;
    CHECK(L.total_bytes >= 4u * L.nsrc && L.total_bytes % 256u == 0 && L.total_bytes - 4u * L.nsrc < 256u);
    for (int k = 0; k < 3; ++k)
        CHECK(L.S[k] == d[k] << shift);
    CHECK(L.wpo == (L.wps + (1u << shift) - 1u) >> shift);
    LodArgs A{};
    lod_args(A, L, d, shift, threshold, work.data(), bits.data(), counts ? cnt.data() : nullptr, summary);

    // k_read_region of the source box: clipped to the world before any load
    const std::vector<uint32_t> src = read_host(h.world(), o, L.S);
    CHECK(src.size() == L.nsrc);
    for (uint64_t i = 0; i < src.size(); ++i)
        ((uint32_t*)work.data())[i] = src[i];

    switch (shift) {
    case 1: run<1>(A, L, split, summary); break;
    case 2: run<2>(A, L, split, summary); break;
    case 3: run<3>(A, L, split, summary); break;
    case 4: run<4>(A, L, split, summary); break;
    default: run<5>(A, L, split, summary); break;
    }
    CHECK(bits[nbits] == guard && cnt[ncells] == (uint16_t)guard);
    if (!counts)
        for (uint64_t i = 0; i < ncells; ++i)
            CHECK(cnt[i] == (uint16_t)guard);

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(summary, 4, 8, out);
    fwrite(bits.data(), 4, nbits, out);
    if (counts)
        fwrite(cnt.data(), 2, ncells, out);
    fclose(out);
    printf("%u set, %u empty, %u full, %u mixed, %llu indices checked, failures %d\n%s\n", summary[2], summary[3], summary[4],
           summary[5], (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
