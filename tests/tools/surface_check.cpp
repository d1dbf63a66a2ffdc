// Host harness of surface extraction (voxelengine_amd/csrc/vxrt_surface.hpp: the face words and face bits of the halo, the
// walk over a row of a mask in both lane mappings, the identical-run test and the records a quad writes), compiled for the
// CPU through tests/tools/hoststub and run one lane at a time, launch by launch.  The harness restates what the kernels of
// vxrt_surface.hip add around that code: the lane mappings' index arithmetic, the two levels of the count scan and the
// summary's totals, which the GPU suite covers.  The world is the oracle's brickmap (oracle/vxo_world.c) of a dense grid,
// laid out as the library holds it in HBM; the halo's bits come from region_row_word, clipped as k_read_region clips.
// Every index the code forms into the workspace or an output is checked against that array's size; the outputs hold
// `capacity` records and a guard after them.  Run by tests/test_surface_host.py, which compares the outputs with
// tests/ref_surface.py.
//
//   surface_check in.bin out.bin
//   in:  i32 op, f, X, Y, Z, origin[3], dims[3], mode, capacity, triangles; X * Y * Z / 32 u32 dense words (vxo_sample_index64)
//   op 0 (extract): out: 16 u32 summary, written x 2 u32 quads, then (triangles) written x 12 i32 and written x 6 u32
//   op 1 (layout only; no world is built): out: u32 accepted by surf_layout with the origin, u32 accepted without it,
//        u64 total_bytes
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_SURF_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_surface.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <vector>
using namespace vxrt;

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: surface_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[14];
    if (!in || fread(hd, 4, 14, in) != 14)
        return 2;
    const int op = hd[0], f = hd[1], X = hd[2], Y = hd[3], Z = hd[4];
    const int32_t o[3] = {hd[5], hd[6], hd[7]}, d[3] = {hd[8], hd[9], hd[10]};
    const uint32_t mode = (uint32_t)hd[11], capacity = (uint32_t)hd[12], triangles = (uint32_t)hd[13];
    SurfLayout L{};
    if (op == 1) {
        fclose(in);
        const uint32_t with = surf_layout(o, d, L) ? 1u : 0u, without = surf_layout(nullptr, d, L) ? 1u : 0u;
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

    if (!surf_layout(o, d, L)) {
        printf("outside the contract\n");
        return 2;
    }
    const uint32_t guard = 0x5A5A5A5Au;
    std::vector<uint8_t> work(L.total_bytes, 0xA5);
    std::vector<uint32_t> quads(2u * (size_t)capacity + 1u, guard), tris(6u * (size_t)capacity + 1u, guard);
    std::vector<int32_t> verts(12u * (size_t)capacity + 1u, (int32_t)guard);
    uint32_t summary[16] = {};
    g_size[kSurfHalo] = L.nhalo;
    g_size[kSurfCounts] = L.nrows;
    g_size[kSurfGroups] = L.ngroups;
    g_size[kSurfQuads] = 2u * (uint64_t)capacity;
    g_size[kSurfVerts] = 12u * (uint64_t)capacity;
    g_size[kSurfTris] = 6u * (uint64_t)capacity;
    CHECK(L.counts >= 4u * L.nhalo && L.groups - L.counts >= 4u * (uint64_t)L.nrows &&
          L.total_bytes - L.groups >= 4u * (uint64_t)L.ngroups && L.counts % 256u == 0 && L.groups % 256u == 0);
    CHECK(L.nrows == 2u * (uint32_t)d[2] * ((uint32_t)d[0] + 2u * (uint32_t)d[1]));
    SurfArgs A{};
    surf_args(A, L, d, mode, work.data(), capacity ? quads.data() : nullptr, capacity, triangles ? verts.data() : nullptr,
              triangles ? tris.data() : nullptr, summary);

    // k_read_region of the halo: clipped to the world before any load
    const std::vector<uint32_t> halo = read_host(h.world(), L.ho, L.hd);
    CHECK(halo.size() == L.nhalo);
    for (uint64_t i = 0; i < halo.size(); ++i)
        ((uint32_t*)(work.data() + L.halo))[i] = halo[i];

    // k_surf_count_yz: one lane per row; k_surf_count_x: lanes (d, z, x), x over whole waves
    std::vector<uint8_t> counted(L.nrows, 0);
    for (uint32_t j = 0; j < L.nryz; ++j) {
        SurfTally t{};
        uint32_t dir = 99u;
        check_index(kSurfCounts, L.nrx + j);
        A.counts[L.nrx + j] = surf_row_yz<false>(A, j, 0u, t, dir);
        counted[L.nrx + j]++;
        CHECK(dir >= 2u && dir < 6u);
        summary[kSurfSumSolid] += t.solid;
        summary[kSurfSumFacesDir + dir] += t.faces;
        summary[kSurfSumQuadsDir + dir] += t.quads;
    }
    const uint32_t x64 = ((uint32_t)d[0] + 63u) / 64u * 64u, nx = 2u * (uint32_t)d[2] * x64;
    for (uint32_t i = 0; i < (nx + 255u) / 256u * 256u; ++i) {
        const uint32_t x = i % x64, q = i / x64, z = q % (uint32_t)d[2], dir = q / (uint32_t)d[2];
        if (dir >= 2u || x >= (uint32_t)d[0])
            continue;
        SurfTally t{};
        const uint32_t r = surf_row_index_x(A, dir, (int32_t)x, (int32_t)z);
        check_index(kSurfCounts, r);
        CHECK(r < L.nrx);
        A.counts[r] = surf_row_x<false>(A, dir, (int32_t)x, (int32_t)z, 0u, t);
        counted[r]++;
        CHECK(t.solid == 0u);
        summary[kSurfSumFacesDir + dir] += t.faces;
        summary[kSurfSumQuadsDir + dir] += t.quads;
    }
    for (uint32_t r = 0; r < L.nrows; ++r)
        CHECK(counted[r] == 1);  // every row has exactly one lane

    // k_surf_scan and k_surf_groups, restated: exclusive within a group of 256 rows, then over the groups
    uint32_t total = 0u;
    for (uint32_t g = 0; g < L.ngroups; ++g) {
        uint32_t sum = 0u;
        for (uint32_t r = g * kSurfGroup; r < (g + 1u) * kSurfGroup && r < L.nrows; ++r) {
            const uint32_t n = A.counts[r];
            A.counts[r] = sum;
            sum += n;
        }
        A.groups[g] = total;
        total += sum;
    }
    for (uint32_t k = 0; k < 6u; ++k)
        summary[kSurfSumFaces] += summary[kSurfSumFacesDir + k];
    summary[kSurfSumQuads] = total;
    summary[kSurfSumWritten] = total < A.capacity ? total : A.capacity;
    CHECK(summary[kSurfSumQuadsDir] + summary[kSurfSumQuadsDir + 1] + summary[kSurfSumQuadsDir + 2] + summary[kSurfSumQuadsDir + 3] +
              summary[kSurfSumQuadsDir + 4] + summary[kSurfSumQuadsDir + 5] == total);

    // k_surf_emit_x, k_surf_emit_yz
    if (A.capacity) {
        for (uint32_t i = 0; i < nx; ++i) {
            const uint32_t x = i % x64, q = i / x64, z = q % (uint32_t)d[2], dir = q / (uint32_t)d[2];
            if (dir >= 2u || x >= (uint32_t)d[0])
                continue;
            const uint32_t pos = surf_row_start(A, surf_row_index_x(A, dir, (int32_t)x, (int32_t)z));
            SurfTally t{};
            if (pos < A.capacity)
                surf_row_x<true>(A, dir, (int32_t)x, (int32_t)z, pos, t);
        }
        for (uint32_t j = 0; j < L.nryz; ++j) {
            const uint32_t pos = surf_row_start(A, L.nrx + j);
            SurfTally t{};
            uint32_t dir;
            if (pos < A.capacity)
                surf_row_yz<true>(A, j, pos, t, dir);
        }
    }
    const uint32_t written = summary[kSurfSumWritten];
    // nothing past the records written is touched
    for (size_t i = 2u * (size_t)written; i < quads.size(); ++i)
        CHECK(quads[i] == guard);
    for (size_t i = triangles ? 12u * (size_t)written : 0u; i < verts.size(); ++i)
        CHECK(verts[i] == (int32_t)guard);
    for (size_t i = triangles ? 6u * (size_t)written : 0u; i < tris.size(); ++i)
        CHECK(tris[i] == guard);

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(summary, 4, 16, out);
    fwrite(quads.data(), 4, 2u * (size_t)written, out);
    if (triangles) {
        fwrite(verts.data(), 4, 12u * (size_t)written, out);
        fwrite(tris.data(), 4, 6u * (size_t)written, out);
    }
    fclose(out);
    printf("%u solid, %u faces, %u quads, %u written, %llu indices checked, failures %d\n%s\n", summary[kSurfSumSolid],
           summary[kSurfSumFaces], total, written, (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
