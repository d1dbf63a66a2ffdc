// Host harness of navigation fields (voxelengine_amd/csrc/vxrt_nav.hpp: the three erosion passes, the goal step, the BFS
// level of one word with the tile lists, the next code of one cell and the path walk of the kernels of vxrt_nav.hip),
// compiled for the CPU through tests/tools/hoststub and run one lane at a time, launch by launch.  The world is the oracle's
// brickmap (oracle/vxo_world.c) of a dense grid, laid out as the library holds it in HBM; the halo's bits come from
// region_row_word, clipped as k_read_region clips.  Every index the nav code forms into the workspace or an output is
// checked against that array's size.  Run by tests/test_nav_host.py, which compares the outputs with tests/ref_nav.py.
//
//   nav_check in.bin out.bin
//   in:  i32 f, X, Y, Z, origin[3], dims[3], width, height, climb, drop, max_dist, ngoals, nstarts, max_steps;
//        ngoals x 3 i32 goals; nstarts x 3 i32 starts; X * Y * Z / 32 u32 dense words (vxo_sample_index64)
//   out: u32 summary[8], region_words u32 walkable, nvox u32 dist, nvox u8 next, nstarts x (max_steps + 1) x 3 i32 cells,
//        nstarts u32 lengths, nstarts u32 status; stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_NAV_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_nav.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <vector>
using namespace vxrt;

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: nav_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[18];
    if (!in || fread(hd, 4, 18, in) != 18)
        return 2;
    const int f = hd[0], X = hd[1], Y = hd[2], Z = hd[3];
    const int32_t o[3] = {hd[4], hd[5], hd[6]}, d[3] = {hd[7], hd[8], hd[9]};
    const int32_t aw = hd[10], ah = hd[11], climb = hd[12], drop = hd[13];
    const uint32_t max_dist = (uint32_t)hd[14], ngoals = (uint32_t)hd[15], nstarts = (uint32_t)hd[16], max_steps = (uint32_t)hd[17];
    std::vector<int32_t> goals(3 * (size_t)ngoals), starts(3 * (size_t)nstarts);
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    if (fread(goals.data(), 4, goals.size(), in) != goals.size() || fread(starts.data(), 4, starts.size(), in) != starts.size() ||
        fread(dense.data(), 4, dense.size(), in) != dense.size())
        return 2;
    fclose(in);

    // the oracle's brickmap in HBM order
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    const HbmWorld h = to_hbm(w);
    vxo_world_free(w);

    NavLayout L;
    if (!nav_layout(d, aw, ah, climb, drop, L)) {
        printf("bad dims or agent\n");
        return 2;
    }
    std::vector<uint32_t> work(L.total_bytes / 4, 0xDEADBEEFu);
    std::vector<uint32_t> walk(L.nb, 0xDEADBEEFu), summary(8, 0u);
    std::vector<uint8_t> next(L.nvox, 0xA5);
    g_size[kNavHalo] = (uint64_t)L.wh * L.hy * L.hz;
    g_size[kNavEx] = (uint64_t)L.wb * L.hy * L.hz;
    g_size[kNavDx] = g_size[kNavFy] = (uint64_t)L.wb * d[1] * L.hz;
    g_size[kNavFree] = g_size[kNavWalk] = g_size[kNavVis] = g_size[kNavFront] = L.nb;
    g_size[kNavDist] = L.nvox;
    g_size[kNavStamp] = 2u * (uint64_t)L.ntiles;
    g_size[kNavMark] = L.ntiles;
    g_size[kNavList] = 3u * (uint64_t)L.ntiles;
    g_size[kNavCtrl] = kNavSlots;
    g_size[kNavNext] = L.nvox;
    g_size[kNavGoals] = 3u * (uint64_t)ngoals;
    g_size[kNavCells] = 3u * (uint64_t)nstarts * (max_steps + 1u);
    g_size[kNavLengths] = nstarts;
    CHECK(L.ex >= g_size[kNavHalo] && L.dx - L.ex >= g_size[kNavEx] && L.fy - L.dx >= g_size[kNavDx] &&
          L.free - L.fy >= g_size[kNavFy] && L.vis - L.free >= L.nb && L.front[0] - L.vis >= L.nb &&
          L.front[1] - L.front[0] >= L.nb && L.dist - L.front[1] >= L.nb && L.stamp - L.dist >= L.nvox &&
          L.list + 3u * (uint64_t)L.ntiles <= L.ctrl && L.ctrl + kNavCtrlWords <= work.size());
    NavArgs A{};
    nav_args(A, L, o, d, aw, ah, climb, drop, goals.data(), ngoals, work.data(), walk.data(), next.data(), nullptr, summary.data());
    // the memsets
    for (uint32_t k = 0; k < kNavCtrlWords; ++k) A.ctrl[k] = 0u;
    for (uint32_t k = 0; k < L.ntiles; ++k) A.mark[k] = 0u;
    for (uint64_t k = 0; k < 2u * (uint64_t)L.ntiles; ++k) A.stamp[k] = 0xFFFFFFFFu;
    for (uint64_t k = 0; k < L.nb; ++k) A.vis[k] = A.front[0][k] = 0u;
    for (uint32_t k = 0; k < L.nvox; ++k) A.dist[k] = kNavUnreached;

    // k_read_region of the halo: clipped to the world before any load
    const int32_t ho[3] = {o[0], o[1] - 1, o[2]}, hdim[3] = {d[0] + aw - 1, (int32_t)L.hy, (int32_t)L.hz};
    const std::vector<uint32_t> halo = read_host(h.world(), ho, hdim);
    for (uint64_t i = 0; i < halo.size(); ++i) {
        check_index(kNavHalo, i);
        work[L.halo + i] = halo[i];
    }

    // k_nav_xpass, k_nav_ypass, k_nav_zpass
    for (uint32_t z = 0; z < L.hz; ++z) for (uint32_t y = 0; y < L.hy; ++y) for (uint32_t xw = 0; xw < L.wb; ++xw)
        nav_xpass_word(A, xw, y, z);
    for (uint32_t z = 0; z < L.hz; ++z) for (uint32_t y = 0; y < (uint32_t)d[1]; ++y) for (uint32_t xw = 0; xw < L.wb; ++xw)
        nav_ypass_word(A, xw, y, z);
    for (uint32_t z = 0; z < (uint32_t)d[2]; ++z) for (uint32_t y = 0; y < (uint32_t)d[1]; ++y) for (uint32_t xw = 0; xw < L.wb; ++xw)
        summary[kNavSumNodes] += nav_zpass_word(A, xw, y, z);
    // k_nav_goals
    for (uint32_t g = 0; g < ngoals; ++g) {
        const int r = nav_goal(A, g);
        ++summary[r ? kNavSumGoalsUsed : kNavSumGoalsIgnored];
        if (r == 2)
            ++summary[kNavSumReached];
    }
    // k_nav_level, level by level: the tile's words lane by lane, then the tile's marks
    uint32_t levels_run = 0;
    for (uint32_t lv = 0; ngoals && lv < max_dist; ++lv) {
        const uint32_t slot = lv % kNavSlots, count = A.ctrl[slot];
        if (!count)
            break;
        ++levels_run;
        A.ctrl[(lv + 2u) % kNavSlots] = 0u;
        summary[kNavSumVisits] += count;
        CHECK(count <= L.ntiles);
        for (uint32_t k = 0; k < count; ++k) {
            check_index(kNavList, (uint64_t)slot * L.ntiles + k);
            const uint32_t t = A.list[(uint64_t)slot * L.ntiles + k];
            CHECK(t < L.ntiles);
            const uint32_t tx = t % L.wb, tr = t / L.wb, ty = tr % L.nty, tz = tr / L.nty;
            int32_t box[4] = {0x7FFFFFFF, -1, 0x7FFFFFFF, -1};
            bool e0 = false, e31 = false;
            uint32_t found = 0;
            for (uint32_t lane = 0; lane < 256; ++lane) {
                const uint32_t y = ty * kNavTileY + (lane & (kNavTileY - 1)), z = tz * kNavTileZ + lane / kNavTileY;
                if (y >= (uint32_t)d[1] || z >= (uint32_t)d[2])
                    continue;
                const uint32_t nw = nav_level_word(A, lv, tx, y, z);
                if (!nw)
                    continue;
                box[0] = box[0] < (int32_t)y ? box[0] : (int32_t)y;
                box[1] = box[1] > (int32_t)y ? box[1] : (int32_t)y;
                box[2] = box[2] < (int32_t)z ? box[2] : (int32_t)z;
                box[3] = box[3] > (int32_t)z ? box[3] : (int32_t)z;
                e0 |= (nw & 1u) != 0;
                e31 |= (nw >> 31) != 0;
                found += (uint32_t)__builtin_popcount(nw);
            }
            check_index(kNavStamp, (uint64_t)((lv + 1u) & 1u) * L.ntiles + t);
            A.stamp[(uint64_t)((lv + 1u) & 1u) * L.ntiles + t] = lv + 1u;
            if (found) {
                summary[kNavSumReached] += found;
                summary[kNavSumMaxDist] = lv + 1u > summary[kNavSumMaxDist] ? lv + 1u : summary[kNavSumMaxDist];
                nav_mark_around(A, lv + 1u, tx, e0, e31, box[0], box[1], box[2], box[3]);
            }
        }
    }
    // k_nav_next, k_nav_finish
    for (uint32_t z = 0; z < (uint32_t)d[2]; ++z) for (uint32_t y = 0; y < (uint32_t)d[1]; ++y) for (uint32_t x = 0; x < (uint32_t)d[0]; ++x) {
        const uint32_t c = nav_cell(A, x, y, z);
        check_index(kNavNext, c);
        A.next[c] = nav_next_cell(A, x, y, z);
        const bool reached = A.dist[c] != kNavUnreached;
        CHECK(reached == (A.next[c] != kNavNone));  // a reachable cell always has a move one level down
    }
    summary[kNavSumLevels] = summary[kNavSumGoalsUsed] ? summary[kNavSumMaxDist] + 1u : 0u;
    summary[kNavSumTiles] = L.ntiles;
    CHECK(summary[kNavSumGoalsUsed] == 0 || levels_run >= summary[kNavSumMaxDist]);

    // k_nav_paths, start by start
    std::vector<int32_t> cells(3u * (size_t)nstarts * (max_steps + 1u) + 1, 0x5A5A5A5A);
    std::vector<uint32_t> lengths(nstarts + 1, 0x5A5A5A5Au), status(nstarts + 1, 0x5A5A5A5Au);
    NavPathArgs P{};
    P.next = next.data();
    P.starts = starts.data();
    P.cells = cells.data();
    P.lengths = lengths.data();
    P.status = status.data();
    P.n = nstarts;
    P.max_steps = max_steps;
    for (int k = 0; k < 3; ++k) {
        P.o[k] = o[k];
        P.d[k] = d[k];
    }
    P.climb = climb;
    P.drop = drop;
    g_size[kNavGoals] = 3u * (uint64_t)nstarts;  // the starts, read through the same check id
    for (uint64_t i = 0; i < nstarts; ++i)
        nav_path(P, i);
    CHECK(cells.back() == 0x5A5A5A5A && lengths.back() == 0x5A5A5A5Au && status.back() == 0x5A5A5A5Au);

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(summary.data(), 4, 8, out);
    fwrite(walk.data(), 4, walk.size(), out);
    fwrite(A.dist, 4, L.nvox, out);
    fwrite(next.data(), 1, next.size(), out);
    fwrite(cells.data(), 4, cells.size() - 1, out);
    fwrite(lengths.data(), 4, nstarts, out);
    fwrite(status.data(), 4, nstarts, out);
    fclose(out);
    printf("%u nodes, %u reached, %u levels, %u of %u tile visits, %llu indices checked, failures %d\n%s\n",
           summary[kNavSumNodes], summary[kNavSumReached], summary[kNavSumLevels], summary[kNavSumVisits], summary[kNavSumTiles],
           (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
