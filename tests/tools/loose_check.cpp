// Host harness of the loose voxels (voxelengine_amd/csrc/vxrt_loose.hpp: the set-up of the blocked, live and first turn
// planes, the FALL, SLIDE and SPREAD passes along both axes, the funnel-shifted output and its tally, of the kernels of
// vxrt_loose.hip), compiled for the CPU through tests/tools/hoststub and run one lane at a time, launch by launch, in the
// order vxrt_loose.hip launches them.  The world is the oracle's brickmap (oracle/vxo_world.c) of a dense grid, laid out as
// the library holds it in HBM; the halo's bits come from region_row_word, clipped as k_read_region clips.  Every index the
// code forms into a plane, the input or the output is checked against that array's size, and after every launch the padding
// bits of the plane it wrote and that the layer lies within Live and off the blocked voxels.  Run by tests/test_loose_host.py,
// which compares the outputs with tests/ref_loose.py.
//
//   loose_check in.bin out.bin
//   in:  i32 op, f, X, Y, Z, origin[3], dims[3], material, steps, edge, phase, shortcut, in_place;
//        X * Y * Z / 32 u32 dense words (vxo_sample_index64); region_words(dims) u32 words of the input layer
//   op 0 (step): out: 12 u32 (vxrt_loose_summary), region_words(dims) u32 words of the new layer
//        shortcut 0: the passes run without the zero-stencil shortcut; in_place 1: the output is the input's buffer
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void check_index(int array, uint64_t index);
#define VXRT_LOOSE_CHECK(array, index) check_index(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_loose.hpp"
#include "hbm_world.h"
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace vxrt;

// the padding bits of every row of a plane are 0
static void check_padding(const LooseArgs& A, const uint32_t* plane)
{
    const uint32_t rem = ((uint32_t)A.d[0] + 2u) & 31u;
    if (!rem)
        return;
    for (uint64_t row = 0; row < (uint64_t)A.hy * A.hz; ++row)
        CHECK((plane[row * A.wh + A.wh - 1u] >> rem) == 0u);
}

// the layer lies within Live and never meets a blocked voxel
static void check_layer(const LooseArgs& A, const uint32_t* plane)
{
    for (uint64_t i = 0; i < A.np; ++i)
        CHECK((plane[i] & ~A.live[i]) == 0u && (plane[i] & A.blocked[i]) == 0u);
}

template <int PASS>
static uint32_t pass_all(const LooseArgs& A, int32_t p, uint32_t t, bool shortcut)
{
    const uint32_t* src = loose_src(A, p);
    uint32_t* dst = loose_dst(A, p);
    CHECK(src != dst && dst != A.blocked && dst != A.live);
    uint32_t moved = 0u;
    for (uint64_t w = 0; w < A.np; ++w)
        moved += shortcut ? loose_pass_lane<PASS, true>(A, src, dst, w, t) : loose_pass_lane<PASS, false>(A, src, dst, w, t);
    check_padding(A, dst);
    check_layer(A, dst);
    return moved;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: loose_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[17];
    if (!in || fread(hd, 4, 17, in) != 17)
        return 2;
    const int f = hd[1], X = hd[2], Y = hd[3], Z = hd[4];
    const int32_t o[3] = {hd[5], hd[6], hd[7]}, d[3] = {hd[8], hd[9], hd[10]};
    vxrt_loose q{};
    q.struct_size = sizeof(vxrt_loose);
    q.material = hd[11];
    q.steps = hd[12];
    q.edge = hd[13];
    q.phase = (uint32_t)hd[14];
    const bool shortcut = hd[15] != 0, in_place = hd[16] != 0;
    LooseLayout L{};
    if (hd[0] != 0 || loose_check(q) != 0 || !loose_layout(o, d, L)) {
        printf("outside the contract\n");
        return 2;
    }
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32);
    const size_t guard = 64;
    std::vector<uint32_t> layer(L.nb + guard, 0x5A5A5A5Au), bits(L.nb + guard, 0x5A5A5A5Au);
    if (fread(dense.data(), 4, dense.size(), in) != dense.size() || fread(layer.data(), 4, L.nb, in) != L.nb)
        return 2;
    fclose(in);
    const std::vector<uint32_t> layer_in(layer.begin(), layer.begin() + L.nb);

    // the oracle's brickmap in HBM order
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    const HbmWorld hw = to_hbm(w);
    vxo_world_free(w);
    const CollideWorld W = hw.world();

    std::vector<uint8_t> work(L.total_bytes + guard, 0xA5);
    uint32_t summary[kLooseSumWords + 1];
    memset(summary, 0x77, sizeof(summary));
    summary[kLooseSumWords] = 0xC0FFEEu;
    g_size[kLoosePlane] = L.np;
    g_size[kLooseIn] = L.nb;
    g_size[kLooseOut] = L.nb;
    // four sections in order, each on a 256-byte boundary and as large as a plane
    const uint64_t pb = 4u * L.np;
    CHECK(L.blocked == 0 && L.live - L.blocked >= pb && L.turn[0] - L.live >= pb && L.turn[1] - L.turn[0] >= pb && L.total_bytes - L.turn[1] >= pb);
    CHECK(L.live % 256u == 0 && L.turn[0] % 256u == 0 && L.turn[1] % 256u == 0 && L.total_bytes % 256u == 0);
    LooseArgs A{};
    loose_args(A, L, W, o, d, q, layer.data(), work.data(), in_place ? layer.data() : bits.data(), summary);

    // k_read_region of the halo: clipped to the world before any load
    const std::vector<uint32_t> halo = read_host(W, L.ho, L.hd);
    CHECK(halo.size() == L.np);
    for (uint64_t i = 0; i < halo.size(); ++i)
        A.blocked[i] = halo[i];

    // k_loose_setup
    for (uint64_t i = 0; i < (L.np > kLooseSumWords ? L.np : (uint64_t)kLooseSumWords); ++i) {
        if (i < kLooseSumWords)
            summary[i] = loose_summary_init((uint32_t)i);
        if (i < L.np)
            loose_setup_lane(A, i);
    }
    check_padding(A, A.blocked);
    check_padding(A, A.live);
    check_padding(A, A.turn[0]);
    check_layer(A, A.turn[0]);

    // `steps` x 2 or 3 x k_loose_pass; the last step's launches tally their movers
    const int32_t per = loose_passes_per_step(q.material), n = loose_passes(q);
    uint64_t before = 0;
    for (uint64_t i = 0; i < L.np; ++i)
        before += (uint64_t)__builtin_popcount(A.turn[0][i]);
    for (int32_t p = 0; p < n; ++p) {
        const uint32_t t = loose_pass_step(q, p);
        const int kind = loose_pass_kind(q.material, p);
        const uint32_t moved = kind == kLooseFall ? pass_all<kLooseFall>(A, p, t, shortcut)
                               : kind == kLooseSlide ? pass_all<kLooseSlide>(A, p, t, shortcut) : pass_all<kLooseSpread>(A, p, t, shortcut);
        if (p >= n - per && moved)
            atom_add(summary + kLooseSumFell + kind, moved);
        // mass: nothing appears, and under VXRT_LOOSE_WALL nothing disappears
        uint64_t after = 0;
        for (uint64_t i = 0; i < L.np; ++i)
            after += (uint64_t)__builtin_popcount(loose_dst(A, p)[i]);
        CHECK(after <= before && (q.edge == kLooseOpen || after == before) && before - after <= moved);
        before = after;
    }

    // k_loose_output and its reduction
    LooseTally t;
    loose_tally_clear(t);
    for (uint64_t i = 0; i < L.nb; ++i)
        loose_output_lane(A, loose_src(A, n), i, t);
    int32_t* box = (int32_t*)summary;
    for (int k = 0; k < 3; ++k) {
        atom_add(summary + kLooseSumIn + k, t.n[k]);
        atom_min(box + kLooseSumMin + k, t.lo[k]);
        atom_max(box + kLooseSumMax + k, t.hi[k]);
    }

    // nothing written behind the output, the input, the workspace or the summary; the output's padding bits are 0; an
    // out-of-place call leaves its input as it was
    const uint32_t* out_words = in_place ? layer.data() : bits.data();
    for (size_t i = 0; i < guard; ++i) {
        CHECK(bits[L.nb + i] == 0x5A5A5A5Au && layer[L.nb + i] == 0x5A5A5A5Au);
        CHECK(work[L.total_bytes + i] == 0xA5);
    }
    CHECK(summary[kLooseSumWords] == 0xC0FFEEu);
    for (uint64_t row = 0; row < (uint64_t)d[1] * d[2]; ++row)
        CHECK((out_words[row * L.mw + L.mw - 1u] & ~row_last_mask(d[0])) == 0u);
    if (!in_place)
        CHECK(memcmp(layer.data(), layer_in.data(), 4u * L.nb) == 0);
    CHECK(summary[kLooseSumAfter] == before && summary[kLooseSumStart] <= summary[kLooseSumIn] && summary[kLooseSumAfter] <= summary[kLooseSumStart]);

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(summary, 4, kLooseSumWords, out);
    fwrite(out_words, 4, L.nb, out);
    fclose(out);
    printf("%u loose in, %u after, %llu indices checked, failures %d\n%s\n", summary[kLooseSumIn], summary[kLooseSumAfter],
           (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
