// Host harness of the box collision queries (voxelengine_amd/csrc/vxrt_collide.hpp: validation, the slab searches, the snap
// arithmetic and the overlap count of k_move_boxes / k_overlap_boxes), compiled for the CPU through tests/tools/hoststub.
// The world is the oracle's brickmap (oracle/vxo_world.c) of a dense grid, laid out as the library holds it in HBM.  Every
// row gather is checked first: the row must lie in the world, every cell record it reads in the cell table and every brick
// row in the pool.  Run by tests/test_collide_host.py, which compares the outputs with tests/ref_collide.py.
//
//   collide_check in.bin out.bin
//   in:  i32 f, X, Y, Z, n, order[3]; X * Y * Z / 32 u32 dense words (oracle layout, vxo_sample_index64); n x 9 f32 bodies
//   out: n x 6 f32 lohi, n u32 move flags, n u32 counts, n u32 overlap flags; stdout: rows gathered, "ALL OK" or "FAILED"
// build: g++ -O1 -std=c++17 -ffp-contract=off -Itests/tools/hoststub -Ioracle tests/tools/collide_check.cpp -x c oracle/vxo_*.c
#include <cstdint>
#include <cstdio>

namespace vxrt {
struct CollideWorld;
}
static void check_row(const vxrt::CollideWorld& W, int64_t x0, int y, int z);
#define VXRT_COLLIDE_CHECK_ROW(W, x0, y, z) check_row(W, x0, y, z)

#include "../../voxelengine_amd/csrc/vxrt_collide.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <vector>
using namespace vxrt;

static uint64_t rows = 0;
static int g_cy = 0;
static uint64_t g_ncells = 0, g_pool_words = 0;
// the table indices region_row_word forms for this row, each checked against the tables' sizes
static void check_row(const CollideWorld& W, int64_t x0, int y, int z)
{
    ++rows;
    CHECK(y >= 0 && y < W.dim[1] && z >= 0 && z < W.dim[2]);
    CHECK(x0 + 31 >= 0 && x0 < W.dim[0]);
    const int64_t bl = x0 >> W.lgf, bh = (x0 + 31) >> W.lgf;
    const int b_lo = bl < 0 ? 0 : (int)bl, b_hi = bh > W.cx - 1 ? W.cx - 1 : (int)bh;
    CHECK((y >> W.lgf) < g_cy);
    const uint64_t row_cells = hbm_index(0, y >> W.lgf, z >> W.lgf, W.cx, W.cz);
    const uint32_t bw = (uint32_t)(W.f * W.f * W.f) >> 5;
    for (int bx = b_lo; bx <= b_hi; ++bx) {
        CHECK(row_cells + (uint64_t)bx < g_ncells);
        if (row_cells + (uint64_t)bx >= g_ncells)
            continue;
        const uint32_t slot = W.meta[row_cells + (uint64_t)bx].x;
        if (slot == kEmptySlot)
            continue;
        const uint32_t rb = (uint32_t)W.f * ((uint32_t)(z & (W.f - 1)) + (uint32_t)W.f * (uint32_t)(y & (W.f - 1)));
        CHECK((uint64_t)slot * bw + (rb >> 5) < g_pool_words);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: collide_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[8];
    if (!in || fread(hd, 4, 8, in) != 8)
        return 2;
    const int f = hd[0], X = hd[1], Y = hd[2], Z = hd[3], n = hd[4];
    const int order[3] = {hd[5], hd[6], hd[7]};
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    std::vector<float> bodies((size_t)n * 9);
    if (fread(dense.data(), 4, dense.size(), in) != dense.size() || fread(bodies.data(), 4, bodies.size(), in) != bodies.size())
        return 2;
    fclose(in);

    // the oracle's brickmap in HBM order
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    const HbmWorld h = to_hbm(w);
    g_cy = h.cd[1];
    g_ncells = h.meta.size();
    g_pool_words = h.pool.size();
    const CollideWorld W = h.world();

    std::vector<float> lohi((size_t)n * 6);
    std::vector<uint32_t> mflags((size_t)n), counts((size_t)n), oflags((size_t)n);
    for (int i = 0; i < n; ++i) {
        mflags[(size_t)i] = collide_move_one(W, &bodies[(size_t)i * 9], order, &lohi[(size_t)i * 6]);
        counts[(size_t)i] = collide_overlap_one(W, &bodies[(size_t)i * 9], oflags[(size_t)i]);
    }
    vxo_world_free(w);
    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(lohi.data(), 4, lohi.size(), out);
    fwrite(mflags.data(), 4, mflags.size(), out);
    fwrite(counts.data(), 4, counts.size(), out);
    fwrite(oflags.data(), 4, oflags.size(), out);
    fclose(out);
    printf("%d bodies, %llu rows gathered, failures %d\n%s\n", n, (unsigned long long)rows, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
