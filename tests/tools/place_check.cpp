// Host harness of the voxel piece queries (voxelengine_amd/csrc/vxrt_place.hpp: validation, the launch shape, the row
// counts, the x windows and the passes of k_place_init / k_place_sweep / k_place_contact / k_place_finish), compiled for the
// CPU through tests/tools/hoststub.  The world is the oracle's brickmap (oracle/vxo_world.c) of a dense grid, laid out as the
// library holds it in HBM.  The passes run task by task and lane by lane, every lane a group of its own, so the minimum and
// the sums of a placement meet in the results' "atomics" (plain read-modify-writes here); the whole batch runs twice, the
// tasks and lanes of the second run in descending order, and the two runs must agree word for word.  Every index the code
// forms is checked: placements, results, piece words (against vxrt_region_words of the piece), and before every world gather
// the row, the cell records and the brick row.  Run by tests/test_place_host.py, which compares the output with
// tests/ref_place.py.
//
//   place_check in.bin out.bin
//   in:  i32 f, X, Y, Z, n, n_pieces, lanes (0: the library's launch shape, else this power of two);
//        X * Y * Z / 32 u32 dense words (oracle layout, vxo_sample_index64); per piece i32 dims[3], then its region words;
//        n x 6 i32 placements
//   out: n x 4 u32 results; stdout: lanes, tasks, gathers, checked indices, "ALL OK" or "FAILED"
// build: g++ -O1 -std=c++17 -ffp-contract=off -Itests/tools/hoststub -Ioracle tests/tools/place_check.cpp -x c oracle/vxo_*.c
#include <cstdint>
#include <cstdio>

namespace vxrt {
struct CollideWorld;
}
static void place_index(int array, uint64_t index);
static void check_row(const vxrt::CollideWorld& W, int64_t x0, int y, int z);
#define VXRT_PLACE_CHECK(array, index) place_index((int)(array), (uint64_t)(index))
#define VXRT_PLACE_CHECK_ROW(W, x0, y, z) check_row(W, x0, y, z)

#include "../../voxelengine_amd/csrc/vxrt_place.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <vector>
using namespace vxrt;

static uint64_t rows = 0, indices = 0;
static int g_cy = 0;
static uint64_t g_ncells = 0, g_pool_words = 0;
static std::vector<uint64_t> g_sizes;  // by array id: placements, results, then every piece's words

static void place_index(int array, uint64_t index)
{
    ++indices;
    CHECK(array >= 0 && (size_t)array < g_sizes.size());
    if (array >= 0 && (size_t)array < g_sizes.size())
        CHECK(index < g_sizes[(size_t)array]);
}

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

// the four passes over the whole batch; `down`: tasks and lanes in descending order
static void run(const PlaceArgs& A, bool down)
{
    const uint64_t n_tasks = A.n * A.tasks;
    for (uint64_t i = 0; i < A.n; ++i)
        place_init(A, down ? A.n - 1 - i : i);
    for (uint64_t t = 0; t < n_tasks; ++t)
        for (uint32_t l = 0; l < A.lanes; ++l)
            place_sweep(A, down ? n_tasks - 1 - t : t, down ? A.lanes - 1 - l : l);
    for (uint64_t t = 0; t < n_tasks; ++t)
        for (uint32_t l = 0; l < A.lanes; ++l)
            place_contact(A, down ? n_tasks - 1 - t : t, down ? A.lanes - 1 - l : l);
    for (uint64_t i = 0; i < A.n; ++i)
        place_finish(A, down ? A.n - 1 - i : i);
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: place_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[7];
    if (!in || fread(hd, 4, 7, in) != 7)
        return 2;
    const int f = hd[0], X = hd[1], Y = hd[2], Z = hd[3], n = hd[4], np = hd[5], lanes = hd[6];
    if (np < 1 || np > (int)kPlaceMaxPieces)
        return 2;
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    if (fread(dense.data(), 4, dense.size(), in) != dense.size())
        return 2;
    std::vector<std::vector<uint32_t>> bits((size_t)np);
    PlaceArgs A{};
    A.n_pieces = (uint32_t)np;
    g_sizes.assign(2 + (size_t)np, 0);
    for (int k = 0; k < np; ++k) {
        int32_t d[3];
        if (fread(d, 4, 3, in) != 3)
            return 2;
        bits[(size_t)k].resize((size_t)region_words(d));
        if (fread(bits[(size_t)k].data(), 4, bits[(size_t)k].size(), in) != bits[(size_t)k].size())
            return 2;
        if (piece_prepare(bits[(size_t)k].data(), d, 0, A.pieces[k]))
            return 2;
        g_sizes[2 + (size_t)k] = bits[(size_t)k].size();
    }
    std::vector<int32_t> pl((size_t)n * 6);
    if (fread(pl.data(), 4, pl.size(), in) != pl.size())
        return 2;
    fclose(in);

    // the oracle's brickmap in HBM order
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    const HbmWorld h = to_hbm(w);
    g_cy = h.cd[1];
    g_ncells = h.meta.size();
    g_pool_words = h.pool.size();

    std::vector<uint32_t> res((size_t)n * 4 + 4, 0xDEADBEEFu), res2 = res;
    A.W = h.world();
    A.placements = pl.data();
    A.n = (uint64_t)n;
    g_sizes[kPlacePlacements] = pl.size();
    g_sizes[kPlaceResults] = (uint64_t)n * 4;
    place_shape(A);
    if (lanes) {  // another launch shape over the same rows
        const uint32_t most = A.lanes * A.tasks;
        A.lanes = (uint32_t)lanes;
        A.tasks = (most + A.lanes - 1) / A.lanes;
    }
    A.results = res.data();
    run(A, false);
    A.results = res2.data();
    run(A, true);
    CHECK(res == res2);
    for (int k = 0; k < 4; ++k)  // the words behind the results
        CHECK(res[(size_t)n * 4 + k] == 0xDEADBEEFu);
    vxo_world_free(w);
    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(res.data(), 4, (size_t)n * 4, out);
    fclose(out);
    printf("%d placements, lanes %u, tasks %u, %llu rows gathered, %llu indices checked, failures %d\n%s\n", n, A.lanes, A.tasks,
           (unsigned long long)rows, (unsigned long long)indices, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
