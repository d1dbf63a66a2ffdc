// Host harness of distance fields (voxelengine_amd/csrc/vxrt_dist.hpp: the x distance from the halo's bits, the slab
// loads, the outward scan and the stores of the two sweeps, the occupancy cells, the live tiles and the tally of the kernels
// of vxrt_dist.hip), compiled for the CPU through tests/tools/hoststub and run one lane at a time, launch by launch and
// workgroup by workgroup.  The world is the oracle's brickmap (oracle/vxo_world.c) of a dense grid, laid out as the library
// holds it in HBM; the halo's bits come from region_row_word, clipped as k_read_region clips.  Every index the code forms
// into the workspace, the output or a slab is checked against that array's size.  Run by tests/test_dist_host.py, which
// compares the outputs with tests/ref_dist.py.
//
//   dist_check in.bin out.bin
//   in:  i32 op, f, X, Y, Z, origin[3], dims[3], radius, mode, skip; X * Y * Z / 32 u32 dense words (vxo_sample_index64)
//   op 0 (field): out: u32 zero, near, far, max_d2, u64 sum_d2, u32 live tiles, tiles, nvox u16 dist2
//   op 1 (layout only; no world is built): out: u32 accepted by dist_layout with the origin, u32 accepted without it,
//        u64 total_bytes
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_DIST_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_dist.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <vector>
using namespace vxrt;

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: dist_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[14];
    if (!in || fread(hd, 4, 14, in) != 14)
        return 2;
    const int op = hd[0], f = hd[1], X = hd[2], Y = hd[3], Z = hd[4];
    const int32_t o[3] = {hd[5], hd[6], hd[7]}, d[3] = {hd[8], hd[9], hd[10]};
    const uint32_t radius = (uint32_t)hd[11], mode = (uint32_t)hd[12], skip = (uint32_t)hd[13];
    DistLayout L{};
    if (op == 1) {
        fclose(in);
        const uint32_t with = dist_layout(o, d, radius, L) ? 1u : 0u, without = dist_layout(nullptr, d, radius, L) ? 1u : 0u;
        const uint64_t bytes = without ? L.total_bytes : 0u;
        FILE* out = fopen(argv[2], "wb");
        if (!out)
            return 2;
        fwrite(&with, 4, 1, out);
        fwrite(&without, 4, 1, out);
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

    if (!dist_layout(o, d, radius, L)) {
        printf("outside the contract\n");
        return 2;
    }
    std::vector<uint8_t> work(L.total_bytes, 0xA5);
    std::vector<uint16_t> dist2((size_t)L.nvox + 1, 0x5A5A);
    uint32_t summary[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    g_size[kDistHalo] = L.nhalo;
    g_size[kDistG2] = L.ng2;
    g_size[kDistOcc] = L.nocc;
    g_size[kDistLive] = L.ntiles;
    g_size[kDistOut] = L.nvox;
    CHECK(L.g2 >= 4u * L.nhalo && L.occ - L.g2 >= 2u * L.ng2 && L.live - L.occ >= L.nocc && L.total_bytes - L.live >= L.ntiles &&
          L.g2 % 256u == 0 && L.occ % 256u == 0 && L.live % 256u == 0);
    DistArgs A{};
    dist_args(A, L, d, radius, mode, work.data(), dist2.data(), summary);
    A.skip = skip;

    // k_read_region of the halo: clipped to the world before any load
    const std::vector<uint32_t> halo = read_host(h.world(), L.ho, L.hd);
    CHECK(halo.size() == L.nhalo);
    for (uint64_t i = 0; i < halo.size(); ++i)
        ((uint32_t*)(work.data() + L.halo))[i] = halo[i];

    // k_dist_occ, k_dist_tiles (the whole neighbourhood as one part)
    for (uint32_t cz = 0; cz < L.ncz; ++cz) for (uint32_t cy = 0; cy < L.ncy; ++cy) for (uint32_t xw = 0; xw < L.wh; ++xw)
        dist_occ_cell(A, xw, cy, cz);
    uint32_t nlive = 0;
    for (uint32_t t = 0; t < L.ntiles; ++t) {
        bool any = false;
        for (uint32_t part = 0; part < 3; ++part)  // three lanes' shares make the whole
            any |= dist_tile_part(A, t, part, 3u);
        CHECK(any == dist_tile_part(A, t, 0u, 1u));
        dist_tile_store(A, t, any);
        nlive += A.live[t];
    }

    // k_dist_ysweep, workgroup by workgroup: the slab's rows, then the outputs
    const uint32_t slab_rows = radius <= 32u ? kDistTile + 64u : (radius <= 96u ? kDistTile + 192u : kDistTile + 2u * kDistMaxRadius);
    std::vector<uint16_t> slab((size_t)slab_rows * kDistTile);
    g_size[kDistSlab] = slab.size();
    for (uint32_t hz = 0; hz < L.hz; ++hz) for (uint32_t ty = 0; ty < L.nty; ++ty) for (uint32_t tx = 0; tx < L.ntx; ++tx) {
        if (!dist_slice_live(A, tx, ty, hz))
            continue;
        const uint32_t left = L.hy - ty * kDistTile, rows = left < kDistTile + 2u * radius ? left : kDistTile + 2u * radius;
        slab.assign(slab.size(), 0x0001);  // a row the code should not read would show as a wrong distance
        g_size[kDistSlab] = (uint64_t)rows * kDistTile;
        for (uint32_t row = 0; row < rows; ++row) for (uint32_t lane = 0; lane < kDistTile; ++lane)
            dist_y_load(A, slab.data(), tx, ty, hz, row, lane);
        for (uint32_t j = 0; j < kDistTile && ty * kDistTile + j < (uint32_t)d[1]; ++j) for (uint32_t lane = 0; lane < kDistTile; ++lane)
            dist_y_store(A, slab.data(), tx, ty, hz, j, lane);
    }

    // k_dist_zsweep, workgroup by workgroup
    const uint32_t nyc = ((uint32_t)d[1] + kDistRows - 1u) / kDistRows;
    uint64_t sum = 0;
    for (uint32_t tz = 0; tz < L.ntz; ++tz) for (uint32_t yc = 0; yc < nyc; ++yc) for (uint32_t tx = 0; tx < L.ntx; ++tx) {
        const uint32_t tile = tx + L.ntx * (yc * kDistRows / kDistTile + L.nty * tz);
        check_index(kDistLive, tile);
        const bool live = A.live[tile] != 0;
        const uint32_t left = L.hz - tz * kDistTile, rows = left < kDistTile + 2u * radius ? left : kDistTile + 2u * radius;
        DistTally t{};
        for (uint32_t y = yc * kDistRows; y < (yc + 1u) * kDistRows && y < (uint32_t)d[1]; ++y) {
            if (live) {
                slab.assign(slab.size(), 0x0001);
                g_size[kDistSlab] = (uint64_t)rows * kDistTile;
                for (uint32_t row = 0; row < rows; ++row) for (uint32_t lane = 0; lane < kDistTile; ++lane)
                    dist_z_load(A, slab.data(), tx, y, tz, row, lane);
            }
            for (uint32_t j = 0; j < kDistTile && tz * kDistTile + j < (uint32_t)d[2]; ++j) for (uint32_t lane = 0; lane < kDistTile; ++lane)
                dist_z_store(A, live ? slab.data() : nullptr, tx, y, tz, j, lane, t);
        }
        CHECK((uint64_t)t.zero + t.near + t.far <= (uint64_t)kDistRows * kDistTile * kDistTile);
        summary[kDistSumZero] += t.zero;
        summary[kDistSumNear] += t.near;
        summary[kDistSumFar] += t.far;
        summary[kDistSumMax] = t.max_d2 > summary[kDistSumMax] ? t.max_d2 : summary[kDistSumMax];
        sum += t.sum;
    }
    CHECK(dist2.back() == 0x5A5A);
    CHECK((uint64_t)summary[kDistSumZero] + summary[kDistSumNear] + summary[kDistSumFar] == L.nvox);

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(summary, 4, 4, out);
    fwrite(&sum, 8, 1, out);
    fwrite(&nlive, 4, 1, out);
    fwrite(&L.ntiles, 4, 1, out);
    fwrite(dist2.data(), 2, L.nvox, out);
    fclose(out);
    printf("%u zero, %u near, %u far, %u of %u tiles live, %llu indices checked, failures %d\n%s\n", summary[kDistSumZero],
           summary[kDistSumNear], summary[kDistSumFar], nlive, L.ntiles, (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
