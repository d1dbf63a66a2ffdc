// Host harness of the voxel materials (voxelengine_amd/csrc/vxrt_material.hpp: the band and the rule of a voxel, the paint
// lookup, the task cut and the march of a field lane, a frame pixel's material, texel and colour), compiled for the CPU
// through tests/tools/hoststub and run task by task and lane by lane.  The world is the oracle's brickmap
// (oracle/vxo_world.c) of a dense grid, laid out as the library holds it in HBM.  The harness restates what vxrt_material.hip
// adds around that code, which the GPU suite covers:
//   the field launch  every lane of every task of material_field_args' cut, the tally of a workgroup (here: one for all)
//                     added to the zeroed summary;
//   the frame launch  frame_launch.h, the primary ray handed in, the summary zeroed, then the lanes' results counted.
// Every index the code forms into an input, an output, the cell table, the brick pool, the paint, the palette, the atlas or
// the tally is checked against that array's size (an array the call was not given has size 0); every array carries a guard
// behind it.  Run by tests/test_material_host.py, which compares with tests/ref_material.py.
//
//   material_check in.bin out.bin
//   in:  i32[24]: mode (0 field, 1 frame), f, X, Y, Z, then
//          field: origin[3], dims[3], seg, paint given, paint origin[3], paint dims[3], misalignment of the output (0 .. 3), n_bands
//          frame: W, H, io, compute units, n_tiles as told, tile_shift, tiles in the atlas, 0, paint origin[3], paint dims[3], 0, n_bands
//                 io: 1 paint given, 2 fb, 4 material AOV, 8 summary, 16 the colour output is the colour input, 32 atlas given
//        n_bands * 5 i32 (y_from, top, under, deep, under_depth); X * Y * Z / 32 u32 dense words (vxo_sample_index64);
//        frame: W * H * 3 f32 colours; W * H u32 keys; W * H i64 hit indices; W * H * 3 f32 ray origins; W * H * 3 f32 ray
//               directions; 256 * 5 u32 palette; (atlas) tiles * T * T u32
//        (paint) one u8 per voxel of the paint box in region order
//   out: field: one u8 per voxel of the box, 260 u32 summary
//        frame: W * H * 3 f32 colours; (fb) W * H u32; (AOV) W * H u8; (summary) 4 u32
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool check_or_report(int array, uint64_t index);
// an index outside its array ends the run before the access
#define VXRT_LF_CHECK(array, index)                       \
    do {                                                  \
        if (!check_or_report(array, (uint64_t)(index))) { \
            printf("FAILED\n");                           \
            exit(1);                                      \
        }                                                 \
    } while (0)
#define VXRT_MAT_CHECK(array, index) VXRT_LF_CHECK(array, index)

#include "../../voxelengine_amd/csrc/vxrt_material.hpp"
#include "hbm_world.h"
using namespace vxrt;
#include "frame_launch.h"

static bool check_or_report(int array, uint64_t index)
{
    const int before = fails;
    check_index(array, index);
    return fails == before;
}

static const uint32_t kGuard = 0x5A5A5A5Au;

static int run_field(const int32_t* hd, const vxrt_material_rules& rules, const CollideWorld& Wd, bool paint_given,
                     std::vector<uint8_t>& paint, const char* out_path)
{
    const int32_t o[3] = {hd[5], hd[6], hd[7]}, d[3] = {hd[8], hd[9], hd[10]};
    const uint32_t seg = (uint32_t)hd[11], mis = (uint32_t)hd[19] & 3u;
    if (material_rules_check(&rules) != 0 || (paint_given && !material_paint_ok(rules)) || material_box_check(o, d) != 0 || seg < 1u) {
        printf("outside the contract\n");
        return 2;
    }
    const uint64_t nvox = (uint64_t)d[0] * d[1] * d[2];
    std::vector<uint32_t> store((nvox + 3u) / 4u + 4u, kGuard);  // 4-byte aligned; the output starts `mis` bytes in
    uint8_t* const out = reinterpret_cast<uint8_t*>(store.data()) + 4u + mis;
    std::vector<uint32_t> sum(kMatTallyWords + 1u, 0u), tally(kMatTallyWords + 1u, 0u);
    sum[kMatTallyWords] = tally[kMatTallyWords] = kGuard;
    const std::vector<uint8_t> paint0 = paint;
    MaterialFieldArgs A{};
    material_field_args(A, rules, o, d, seg, out);
    A.paint = paint_given ? paint.data() : nullptr;
    A.summary = sum.data();
    g_size[kMatPaint] = paint_given ? (uint64_t)rules.paint_dims[0] * rules.paint_dims[1] * rules.paint_dims[2] : 0u;
    g_size[kMatOut] = nvox;
    g_size[kMatTally] = kMatTallyWords;
    CHECK(A.dword == ((d[0] % 4 == 0 && mis == 0u) ? 1u : 0u));
    CHECK(A.tasks >= 1u && A.tasks == (uint64_t)A.nxc * A.nys * A.nzg && (uint64_t)A.nys * seg >= (uint64_t)d[1] &&
          (uint64_t)(A.nys - 1u) * seg < (uint64_t)d[1] && (uint64_t)A.nxc * 256u >= (uint64_t)d[0] && (A.nxc == 1u || A.lgL == 6u) &&
          (4u << A.lgL) * (uint64_t)A.nxc >= (uint64_t)d[0] && (uint64_t)A.nzg * (64u >> A.lgL) >= (uint64_t)d[2]);
    // the launch of vxrt_material.hip, restated: four tasks per workgroup, 64 lanes per task
    const uint64_t blocks = (A.tasks + 3u) / 4u;
    for (uint64_t b = 0; b < blocks; ++b)
        for (uint32_t tid = 0; tid < 256u; ++tid) {
            const uint64_t task = b * 4u + (tid >> 6);
            if (task < A.tasks)
                mat_field_lane(A, Wd, task, tid & 63u, tally.data());
        }
    for (uint32_t i = 0; i < kMatTallyWords; ++i)
        sum[i] += tally[i];
    // nothing around the box's bytes touched (a byte of the box that was not written stays 0x5A = 90, an id no case uses: the
    // comparison with the restatement tells)
    const uint8_t* raw = reinterpret_cast<const uint8_t*>(store.data());
    for (uint64_t i = 0; i < 4u + mis; ++i)
        CHECK(raw[i] == 0x5A);
    for (uint64_t i = 4u + mis + nvox; i < 4u * store.size(); ++i)
        CHECK(raw[i] == 0x5A);
    CHECK(sum[kMatTallyWords] == kGuard && tally[kMatTallyWords] == kGuard && paint == paint0 && sum[3] == 0u);
    uint64_t total = 0;
    for (uint32_t i = 4; i < kMatTallyWords; ++i)
        total += sum[i];
    CHECK(total == nvox && sum[0] + sum[4] == nvox && sum[1] <= sum[0] && sum[2] <= sum[0]);
    FILE* f = fopen(out_path, "wb");
    if (!f)
        return 2;
    fwrite(out, 1, nvox, f);
    fwrite(sum.data(), 4, kMatTallyWords, f);
    fclose(f);
    return 0;
}

static int run_frame(FILE* in, const int32_t* hd, const vxrt_material_rules& rules, const CollideWorld& Wd, const HbmWorld& h,
                     std::vector<uint8_t>& paint, const char* out_path)
{
    const uint32_t W = (uint32_t)hd[5], H = (uint32_t)hd[6], io = (uint32_t)hd[7], cus = (uint32_t)hd[8];
    const bool paint_given = io & 1u, fb = io & 2u, aov = io & 4u, summary = io & 8u, alias = io & 16u, atlas_given = io & 32u;
    vxrt_material_frame_params p{};
    p.struct_size = sizeof p;
    p.n_tiles = (uint32_t)hd[9];
    p.tile_shift = (uint32_t)hd[10];
    if (material_frame_check(W, H, &p, &rules, paint_given) != 0) {
        printf("outside the contract\n");
        return 2;
    }
    const uint64_t n = (uint64_t)W * H, texels = (uint64_t)hd[11] << (2u * p.tile_shift);
    float guardf;
    memcpy(&guardf, &kGuard, 4);
    std::vector<float> cin(3u * n + 1u), cout_(3u * n + 1u, guardf), o(3u * n), d(3u * n);
    std::vector<uint32_t> keys(n + 1u), fbv(n + 1u, kGuard), sum(5u, kGuard), pal(256u * 5u + 1u), atl(texels + 1u);
    std::vector<long long> hit(n + 1u);
    std::vector<uint8_t> av(n + 1u, 0x5A);
    if (fread(cin.data(), 4, 3u * n, in) != 3u * n || fread(keys.data(), 4, n, in) != n || fread(hit.data(), 8, n, in) != n ||
        fread(o.data(), 4, 3u * n, in) != 3u * n || fread(d.data(), 4, 3u * n, in) != 3u * n || fread(pal.data(), 4, 1280, in) != 1280 ||
        (atlas_given && fread(atl.data(), 4, texels, in) != texels))
        return 2;
    const uint64_t pvox = paint_given ? (uint64_t)rules.paint_dims[0] * rules.paint_dims[1] * rules.paint_dims[2] : 0u;
    if (paint_given && fread(paint.data(), 1, pvox, in) != pvox)
        return 2;
    cin[3u * n] = guardf;
    keys[n] = pal[1280] = atl[texels] = kGuard;
    hit[n] = 0x5A5A5A5A5A5A5A5All;
    const std::vector<float> cin0 = cin;
    const std::vector<uint32_t> keys0 = keys, pal0 = pal, atl0 = atl;
    const std::vector<long long> hit0 = hit;
    const std::vector<uint8_t> paint0 = paint;
    const std::vector<uint2> meta0 = h.meta;
    const std::vector<uint32_t> pool0 = h.pool;

    static_assert(sizeof(vxrt_material) == 20, "palette entry");
    MaterialFrameArgs A{};
    A.rules = rules;
    A.color_in = cin.data();
    A.keys = keys.data();
    A.hit = hit.data();
    A.paint = paint_given ? paint.data() : nullptr;
    A.palette = reinterpret_cast<const vxrt_material*>(pal.data());
    A.atlas = atlas_given ? atl.data() : nullptr;
    A.color_out = alias ? cin.data() : cout_.data();
    A.fb = fb ? fbv.data() : nullptr;
    A.aov = aov ? av.data() : nullptr;
    A.summary = summary ? sum.data() : nullptr;
    A.W = W;
    A.H = H;
    A.n_tiles = p.n_tiles;
    A.tile_shift = p.tile_shift;
    g_size[kLfColorIn] = 3u * n;
    g_size[kLfKeys] = n;
    g_size[kLfHit] = n;
    g_size[kLfColorOut] = 3u * n;
    g_size[kLfFb] = fb ? n : 0u;
    g_size[kMatAov] = aov ? n : 0u;
    g_size[kMatPaint] = pvox;
    g_size[kMatPalette] = 256u;
    g_size[kMatAtlas] = atlas_given ? texels : 0u;

    uint32_t count[4] = {0u, 0u, 0u, 0u};
    frame_launch(W, H, summary, cus, [&](uint32_t x, uint32_t y, uint64_t at) {
        const uint32_t bits = mat_pixel(A, Wd, x, y, &o[3u * at], &d[3u * at]);
        CHECK(bits < 16u && ((bits & kMatHitBit) != 0u || bits == 0u));
        for (int k = 0; k < 4; ++k)
            count[k] += (bits >> k) & 1u;
    });
    if (summary)
        for (int k = 0; k < 4; ++k)
            sum[k] = count[k];

    // guards, and the inputs unchanged (the colours: unless they are the output)
    uint32_t g[2];
    memcpy(&g[0], &cin[3u * n], 4);
    memcpy(&g[1], &cout_[3u * n], 4);
    CHECK(g[0] == kGuard && g[1] == kGuard && fbv[n] == kGuard && sum[4] == kGuard && av[n] == 0x5A);
    CHECK(keys == keys0 && hit == hit0 && paint == paint0 && pal == pal0 && atl == atl0);
    CHECK(memcmp(h.meta.data(), meta0.data(), meta0.size() * sizeof(uint2)) == 0 && h.pool == pool0);
    if (!alias)
        CHECK(memcmp(cin.data(), cin0.data(), 12u * n) == 0);
    if (alias)
        for (uint64_t i = 0; i < 3u * n; ++i)
            CHECK(memcmp(&cout_[i], &kGuard, 4) == 0);
    if (!fb)
        for (uint64_t i = 0; i < n; ++i)
            CHECK(fbv[i] == kGuard);
    if (!aov)
        for (uint64_t i = 0; i < n; ++i)
            CHECK(av[i] == 0x5A);
    if (!summary)
        for (int i = 0; i < 4; ++i)
            CHECK(sum[i] == kGuard);

    FILE* f = fopen(out_path, "wb");
    if (!f)
        return 2;
    fwrite(alias ? cin.data() : cout_.data(), 4, 3u * n, f);
    if (fb)
        fwrite(fbv.data(), 4, n, f);
    if (aov)
        fwrite(av.data(), 1, n, f);
    if (summary)
        fwrite(sum.data(), 4, 4, f);
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: material_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[24];
    if (!in || fread(hd, 4, 24, in) != 24)
        return 2;
    const int mode = hd[0], f = hd[1], X = hd[2], Y = hd[3], Z = hd[4];
    const uint32_t nb = (uint32_t)hd[20];
    if (nb > 8u)
        return 2;
    vxrt_material_rules rules{};
    rules.struct_size = sizeof rules;
    rules.n_bands = nb;
    for (uint32_t i = 0; i < nb; ++i) {
        int32_t b[5];
        if (fread(b, 4, 5, in) != 5)
            return 2;
        rules.bands[i].y_from = b[0];
        rules.bands[i].top = (uint8_t)b[1];
        rules.bands[i].under = (uint8_t)b[2];
        rules.bands[i].deep = (uint8_t)b[3];
        rules.bands[i].under_depth = (uint8_t)b[4];
    }
    for (int k = 0; k < 3; ++k) {
        rules.paint_origin[k] = hd[13 + k];
        rules.paint_dims[k] = hd[16 + k];
    }
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    if (fread(dense.data(), 4, dense.size(), in) != dense.size())
        return 2;
    const bool paint_given = mode == 0 ? hd[12] != 0 : (hd[7] & 1) != 0;
    const uint64_t pvox = paint_given && material_paint_ok(rules) ? (uint64_t)rules.paint_dims[0] * rules.paint_dims[1] * rules.paint_dims[2] : 0u;
    std::vector<uint8_t> paint(pvox + 16u, 0x5A);
    if (mode == 0 && paint_given && fread(paint.data(), 1, pvox, in) != pvox)
        return 2;
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    if (!w)
        return 2;
    const HbmWorld h = to_hbm(w);
    vxo_world_free(w);
    const CollideWorld Wd = h.world();
    g_size[kLfMeta] = h.meta.size();
    g_size[kLfPool] = h.pool.size();
    const int rc = mode == 0 ? run_field(hd, rules, Wd, paint_given, paint, argv[2]) : run_frame(in, hd, rules, Wd, h, paint, argv[2]);
    fclose(in);
    if (rc)
        return rc;
    printf("%llu indices checked, failures %d\n%s\n", (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
