// Host harness of floating-island detection (voxelengine_amd/csrc/vxrt_islands.hpp: run starts, the tile-local union, the
// border merge, flatten with the anchor test, the island scan, the table rows and the per-voxel output of the kernels of
// vxrt_islands.hip), compiled for the CPU through tests/tools/hoststub and run one lane at a time, launch by launch.  The
// world is the oracle's brickmap (oracle/vxo_world.c) of a dense grid, laid out as the library holds it in HBM; the box's
// bits come from region_row_word, clipped as k_read_region clips.  Every index the island code forms into the workspace,
// the LDS tile or an output is checked against that array's size.  Run by tests/test_islands_host.py, which compares the
// outputs with tests/ref_islands.py.
//
//   islands_check in.bin out.bin
//   in:  i32 f, X, Y, Z, origin[3], dims[3], anchors, max_islands; X * Y * Z / 32 u32 dense words (vxo_sample_index64)
//   out: u32 summary[3], nvox u32 labels, region_words u32 floating, min(islands, max_islands) x 8 i32 rows;
//        stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_ISL_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_islands.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <vector>
using namespace vxrt;

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: islands_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[12];
    if (!in || fread(hd, 4, 12, in) != 12)
        return 2;
    const int f = hd[0], X = hd[1], Y = hd[2], Z = hd[3];
    const int32_t o[3] = {hd[4], hd[5], hd[6]}, d[3] = {hd[7], hd[8], hd[9]};
    const uint32_t anchors = (uint32_t)hd[10], max_islands = (uint32_t)hd[11];
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    if (fread(dense.data(), 4, dense.size(), in) != dense.size())
        return 2;
    fclose(in);

    // the oracle's brickmap in HBM order
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    const HbmWorld h = to_hbm(w);
    vxo_world_free(w);

    IslandsLayout L;
    if (!islands_layout(d, L)) {
        printf("bad dims\n");
        return 2;
    }
    std::vector<uint32_t> work(L.total_bytes / 4, 0xDEADBEEFu);
    std::vector<uint32_t> floating(L.nbits, 0xDEADBEEFu), labels(L.nvox, 0xDEADBEEFu), summary(3, 0u);
    std::vector<int32_t> table((size_t)max_islands * 8 + 1, 0x5A5A5A5A);
    g_size[kIslBits] = L.nbits;
    g_size[kIslParent] = L.nvox;
    g_size[kIslRoots] = g_size[kIslAnchor] = g_size[kIslPrefix] = L.nwords;
    g_size[kIslBlocks] = L.nblocks;
    g_size[kIslFloating] = L.nbits;
    g_size[kIslLabels] = L.nvox;
    g_size[kIslTable] = max_islands;
    g_size[kIslTile] = kIslTileVoxels;
    CHECK(L.blocks + L.nblocks <= work.size() && L.prefix + L.nwords <= L.blocks && L.anchor + L.nwords <= L.prefix &&
          L.roots + L.nwords <= L.anchor && L.parent + L.nvox <= L.roots && L.nbits <= L.parent);
    IslandsArgs A{};
    islands_args(A, L, o, d, anchors, work.data(), floating.data(), labels.data(), table.data(), max_islands, summary.data());
    for (uint32_t k = 0; k < L.nwords; ++k)
        A.anchor[k] = 0u;  // the memset

    // k_read_region: the box's words, clipped to the world before any load
    const std::vector<uint32_t> box = read_host(h.world(), o, d);
    std::copy(box.begin(), box.end(), work.data() + L.bits);

    // k_isl_local, tile by tile: the three phases of the workgroup, lane by lane
    const uint32_t ntx = L.wpr, nty = (d[1] + kIslTileY - 1) / kIslTileY, ntz = (d[2] + kIslTileZ - 1) / kIslTileZ;
    std::vector<uint32_t> lp(kIslTileVoxels), rows(kIslTileRows);
    for (uint32_t tz = 0; tz < ntz; ++tz) for (uint32_t ty = 0; ty < nty; ++ty) for (uint32_t tx = 0; tx < ntx; ++tx) {
        for (uint32_t r = 0; r < kIslTileRows; ++r)
            rows[r] = isl_tile_row(A, tx, ty, tz, r);
        for (uint32_t r = 0; r < kIslTileRows; ++r)
            for (uint32_t x = 0; x < 32; ++x)
                isl_tile_init_voxel(lp.data(), rows[r], x, r);
        for (uint32_t r = 0; r < kIslTileRows; ++r)
            isl_tile_union_row(lp.data(), rows.data(), r);
        for (uint32_t r = 0; r < kIslTileRows; ++r)
            for (uint32_t x = 0; x < 32; ++x) {
                uint32_t g, val;
                if (isl_tile_parent(A, lp.data(), rows.data(), tx, ty, tz, x, r, g, val)) {
                    check_index(kIslParent, g);
                    A.parent[g] = val;
                    CHECK(val == kIslEmpty || val <= g);
                }
            }
    }
    // k_isl_merge
    for (uint64_t wi = 0; wi < L.nbits; ++wi) {
        const uint32_t row = (uint32_t)(wi / L.wpr);
        isl_merge_word(A, (uint32_t)(wi % L.wpr), row % (uint32_t)d[1], row / (uint32_t)d[1]);
    }
    // k_isl_flatten: 64 indices per wave, the root words as the ballots
    for (uint32_t q = 0; q < L.nwords / 2; ++q) {
        uint64_t m = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t i = 64u * q + lane;
            uint32_t root = 0;
            bool anchor = false, solid = false;
            if (i < L.nvox)
                solid = isl_flatten_voxel(A, i, root, anchor);
            if (solid && root == i)
                m |= 1ull << lane;
            if (solid && anchor)
                isl_mark_anchor(A, root);
        }
        check_index(kIslRoots, 2u * q + 1u);
        A.roots[2u * q] = (uint32_t)m;
        A.roots[2u * q + 1u] = (uint32_t)(m >> 32);
        summary[0] += (uint32_t)__builtin_popcountll(m);
    }
    // k_isl_scan_blocks, k_isl_scan_top
    for (uint32_t b = 0; b < L.nblocks; ++b) {
        uint32_t ex = 0;
        for (uint32_t k = 0; k < kIslScanBlock && b * kIslScanBlock + k < L.nwords; ++k) {
            const uint32_t wd = b * kIslScanBlock + k, iw = isl_island_word(A, wd);
            A.roots[wd] = iw;
            A.prefix[wd] = ex;
            ex += (uint32_t)__builtin_popcount(iw);
        }
        A.blocks[b] = ex;
    }
    uint32_t total = 0;
    for (uint32_t b = 0; b < L.nblocks; ++b) {
        const uint32_t v = A.blocks[b];
        A.blocks[b] = total;
        total += v;
    }
    summary[1] = total;
    // k_isl_rows
    if (A.table)
        for (uint32_t wd = 0; wd < L.nwords; ++wd) {
            uint32_t iw = A.roots[wd], rank = A.blocks[wd / kIslScanBlock] + A.prefix[wd];
            for (; iw && rank < A.max_islands; iw &= iw - 1u, ++rank) {
                const uint32_t r = 32u * wd + (uint32_t)__builtin_ctz(iw);
                CHECK(isl_rank(A, r) == rank);
                isl_init_row(A, rank, r);
            }
        }
    // k_isl_output, voxel by voxel
    for (uint64_t wi = 0; wi < L.nbits; ++wi) {
        const uint32_t xw = (uint32_t)(wi % L.wpr), row = (uint32_t)(wi / L.wpr);
        const uint32_t y = row % (uint32_t)d[1], z = row / (uint32_t)d[1];
        uint32_t word = 0;
        for (uint32_t b = 0; b < 32; ++b) {
            const uint32_t x = 32u * xw + b;
            uint32_t rank = 0xFFFFFFFFu;
            if (x >= (uint32_t)d[0] || !isl_voxel_island(A, A.bits[wi], x, y, z, rank))
                continue;
            word |= 1u << b;
            ++summary[2];
            if (rank != 0xFFFFFFFFu) {
                const int32_t g[3] = {o[0] + (int32_t)x, o[1] + (int32_t)y, o[2] + (int32_t)z};
                isl_add_to_row(A, rank, 1u, g, g);
            }
        }
        check_index(kIslFloating, wi);
        A.floating[wi] = word;
    }

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    const uint32_t nrows = summary[1] < max_islands ? summary[1] : max_islands;
    fwrite(summary.data(), 4, 3, out);
    fwrite(labels.data(), 4, labels.size(), out);
    fwrite(floating.data(), 4, floating.size(), out);
    fwrite(table.data(), 4, (size_t)nrows * 8, out);
    fclose(out);
    CHECK(table[(size_t)max_islands * 8] == 0x5A5A5A5A);  // nothing past the table
    printf("%u components, %u islands, %llu indices checked, failures %d\n%s\n", summary[0], summary[1],
           (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
