// Host harness of the voxel edit logic (voxelengine_amd/csrc/vxrt_edit.hpp: op clipping, the per-brick op filter, voxel
// membership, extent packing -- the functions k_edit_bricks runs -- and the slot plan of vxrt_edit_voxels), compiled for
// the CPU through tests/tools/hoststub and compared with the oracle (oracle/vxo_edit.c: vxo_apply_edits;
// oracle/vxo_world.c: the brickmap builder).  Run by tests/test_edit_host.py.
// build: g++ -O1 -std=c++17 -Itests/tools/hoststub -Ioracle tests/tools/edit_check.cpp -x c oracle/vxo_*.c -lm -lpthread
#include "../../voxelengine_amd/csrc/vxrt_device.hpp"
#include "../../voxelengine_amd/csrc/vxrt_edit.hpp"
extern "C" {
#include "vxo.h"
#include "vxo_edit.h"
}
#include "hbm_world.h"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace vxrt;

// what k_edit_bricks computes for the brick at cell (bx, by, bz), one voxel at a time
static void edit_brick_host(const std::vector<EditOpDev>& ops, const std::vector<uint32_t>& old, int bx, int by, int bz, int f,
                            std::vector<uint32_t>& img, uint32_t& ext, bool& changed)
{
    const int b0[3] = {bx * f, by * f, bz * f};
    size_t first = 0;
    for (size_t k = 0; k < ops.size(); ++k)
        if (edit_meets_brick(ops[k], b0, f) && edit_covers_brick(ops[k], b0, f))
            first = k;
    std::vector<size_t> list;
    for (size_t k = first; k < ops.size(); ++k)
        if (edit_meets_brick(ops[k], b0, f))
            list.push_back(k);
    const int fshift = brick_shift(f);
    img.assign(old.size(), 0u);
    int mn[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, mx[3] = {-1, -1, -1};
    for (uint32_t o = 0; o < (uint32_t)(f * f * f); ++o) {
        const int lx = (int)(o & (uint32_t)(f - 1)), lz = (int)((o >> fshift) & (uint32_t)(f - 1)), ly = (int)(o >> (2 * fshift));
        bool solid = ((old[o >> 5] >> (o & 31u)) & 1u) != 0u;
        for (size_t k : list)
            if (edit_covers(ops[k], b0[0] + lx, b0[1] + ly, b0[2] + lz))
                solid = ops[k].value != 0;
        if (solid) {
            img[o >> 5] |= 1u << (o & 31u);
            mn[0] = std::min(mn[0], lx); mn[1] = std::min(mn[1], ly); mn[2] = std::min(mn[2], lz);
            mx[0] = std::max(mx[0], lx); mx[1] = std::max(mx[1], ly); mx[2] = std::max(mx[2], lz);
        }
    }
    ext = edit_pack_extents(mn, mx);
    changed = img != old;
}

static vxo_edit_op random_op(std::mt19937& rng, int X, int Y, int Z)
{
    vxo_edit_op o{};
    o.kind = (int)(rng() % 2);
    o.value = (int)(rng() % 2);
    const int dim[3] = {X, Y, Z};
    if (o.kind == 0) {
        for (int a = 0; a < 3; ++a) {
            const int lo = (int)(rng() % (dim[a] + 16)) - 8, len = (int)(rng() % (dim[a] / 2 + 1)) - 2;
            o.a[a] = lo;
            o.b[a] = lo + len;
        }
    } else {
        for (int a = 0; a < 3; ++a)
            o.a[a] = (int)(rng() % (dim[a] + 20)) - 10;
        o.b[0] = (int)(rng() % (X / 3 + 2));
    }
    return o;
}

// per-brick logic against the oracle: random worlds, random op lists, every brick cell of the world
static void check_bricks(int f, int S, int rounds, unsigned seed)
{
    std::mt19937 rng(seed);
    const int X = S, Y = S, Z = S, cx = X / f, cy = Y / f, cz = Z / f;
    size_t bricks = 0, changed_total = 0;
    for (int r = 0; r < rounds; ++r) {
        std::vector<uint32_t> dense((size_t)X * Y * Z / 32, 0u);
        const double dens = (r % 3) * 0.2;
        for (int z = 0; z < Z; ++z) for (int y = 0; y < Y; ++y) for (int x = 0; x < X; ++x)
            if ((rng() % 1000) < dens * 1000) vxo_bit_set(dense.data(), vxo_sample_index64(x, y, z, X, Y), 1);
        const int nops = 1 + (int)(rng() % 12);
        std::vector<vxo_edit_op> ops;
        std::vector<EditOpDev> dev;
        for (int k = 0; k < nops; ++k) {
            ops.push_back(random_op(rng, X, Y, Z));
            EditOpDev d;
            bool noop = false;
            CHECK(edit_prepare(ops.back().kind, ops.back().value, ops.back().a, ops.back().b, X, Y, Z, d, noop) == 0);
            if (!noop)
                dev.push_back(d);
        }
        vxo_world* before = vxo_build_brickmap(dense.data(), X, Y, Z, f);
        std::vector<uint32_t> edited = dense;
        CHECK(vxo_apply_edits(edited.data(), X, Y, Z, ops.data(), ops.size()) == 0);
        vxo_world* after = vxo_build_brickmap(edited.data(), X, Y, Z, f);
        for (int bz = 0; bz < cz; ++bz) for (int by = 0; by < cy; ++by) for (int bx = 0; bx < cx; ++bx) {
            const uint32_t t = ref_tiled_index(bx, by, bz, cx / 8 ? cx / 8 : 1, cy / 8 ? cy / 8 : 1);
            std::vector<uint32_t> img;
            uint32_t ext = 0;
            bool changed = false;
            edit_brick_host(dev, hbm_brick(before, before->brick_slot[t], f), bx, by, bz, f, img, ext, changed);
            const std::vector<uint32_t> want = hbm_brick(after, after->brick_slot[t], f);
            uint32_t want_ext = 0;
            if (after->brick_slot[t] != VXO_EMPTY_SLOT)
                for (int k = 0; k < 6; ++k) want_ext |= (uint32_t)(int)after->bounds[t * 6 + k] << (5 * k);
            CHECK(img == want);
            CHECK(ext == want_ext);
            ++bricks;
            changed_total += changed;
        }
        vxo_world_free(before);
        vxo_world_free(after);
    }
    printf("bricks f=%d: %zu checked, %zu changed, failures %d\n", f, bricks, changed_total, fails);
}

// the slot plan: frees first, the lowest free slot next, the high-water mark last; deterministic
static void check_plan()
{
    const uint32_t E = 0xFFFFFFFFu;
    std::set<uint32_t> fr;
    EditPlan P;
    // cells 0..3 hold slots 0..3; 1 and 2 become empty, a new cell appears: it takes slot 1
    {
        const uint32_t old[5] = {0, 1, 2, 3, E};
        const uint8_t fl[5] = {0, 2, 2, 3, 3};
        edit_plan_slots(old, fl, 5, fr, 4, P);
        CHECK(P.new_slot[0] == kEditKeep && P.new_slot[1] == E && P.new_slot[2] == E && P.new_slot[3] == 3 && P.new_slot[4] == 1);
        CHECK(P.created == 1 && P.freed == 2 && P.changed == 4 && P.nslots == 4);
        CHECK(P.zero.size() == 1 && P.zero[0] == 2 && fr.size() == 1 && *fr.begin() == 2);
    }
    // three new cells: slot 2 from the free list, then 4 and 5 past the high-water mark
    {
        const uint32_t old[3] = {E, E, E};
        const uint8_t fl[3] = {3, 3, 3};
        edit_plan_slots(old, fl, 3, fr, 4, P);
        CHECK(P.new_slot[0] == 2 && P.new_slot[1] == 4 && P.new_slot[2] == 5 && P.nslots == 6 && fr.empty() && P.zero.empty());
    }
    // an unchanged call plans nothing
    {
        const uint32_t old[2] = {E, 7};
        const uint8_t fl[2] = {0, 1};
        edit_plan_slots(old, fl, 2, fr, 6, P);
        CHECK(P.changed == 0 && P.created == 0 && P.freed == 0 && P.nslots == 6 && P.new_slot[0] == kEditKeep && P.new_slot[1] == kEditKeep);
    }
    // determinism and reuse: clear k bricks, set them again: the same slots, no growth of the high-water mark
    {
        std::set<uint32_t> a, b;
        std::vector<uint32_t> old(64), none(64, E);
        std::vector<uint8_t> clear(64, 2), set(64, 3);
        for (int i = 0; i < 64; ++i) old[i] = (uint32_t)(63 - i);
        EditPlan P1, P2, P3;
        edit_plan_slots(old.data(), clear.data(), 64, a, 64, P1);
        edit_plan_slots(old.data(), clear.data(), 64, b, 64, P2);
        CHECK(P1.zero == P2.zero && a == b && P1.freed == 64 && a.size() == 64);
        edit_plan_slots(none.data(), set.data(), 64, a, P1.nslots, P3);
        CHECK(P3.created == 64 && P3.nslots == 64 && a.empty());
        for (int i = 0; i < 64; ++i) CHECK(P3.new_slot[i] == (uint32_t)i);  // lowest free slot first, cell order
    }
    // undo (a call that fails after planning): the free list as it was, including slots reused within the call
    {
        std::set<uint32_t> f0 = {3, 9, 12}, f = f0;
        const uint32_t old[4] = {5, E, E, 7};
        const uint8_t fl[4] = {2, 3, 3, 3};
        EditPlan Pu;
        edit_plan_slots(old, fl, 4, f, 20, Pu);
        CHECK(Pu.new_slot[1] == 3 && Pu.new_slot[2] == 5 && Pu.new_slot[0] == E && Pu.zero.empty());
        edit_plan_undo(Pu, f);
        CHECK(f == f0);
    }
    // growth: 1.5x or what is needed
    CHECK(edit_grown_capacity(100, 101) == 150);
    CHECK(edit_grown_capacity(100, 400) == 400);
    CHECK(edit_grown_capacity(0, 3) == 3);
    CHECK(edit_grown_capacity(1, 2) == 2);
    // validation: what vxrt_edit_voxels refuses, and the no-op shapes
    {
        EditOpDev d;
        bool noop;
        const int32_t a[3] = {4, 4, 4}, b0[3] = {8, 8, 8}, r1[3] = {1, 0, 0}, rneg[3] = {-1, 0, 0}, rbad[3] = {1, 1, 0};
        CHECK(edit_prepare(2, 1, a, b0, 16, 16, 16, d, noop) != 0);
        CHECK(edit_prepare(0, 2, a, b0, 16, 16, 16, d, noop) != 0);
        CHECK(edit_prepare(1, 1, a, rneg, 16, 16, 16, d, noop) != 0);
        CHECK(edit_prepare(1, 1, a, rbad, 16, 16, 16, d, noop) != 0);
        CHECK(edit_prepare(1, 0, a, r1, 16, 16, 16, d, noop) == 0 && !noop);
        CHECK(edit_prepare(0, 1, b0, a, 16, 16, 16, d, noop) == 0 && noop);  // a > b: empty box
        const int32_t far[3] = {100, 4, 4}, farb[3] = {200, 8, 8};
        CHECK(edit_prepare(0, 1, far, farb, 16, 16, 16, d, noop) == 0 && noop);  // wholly outside
        // a huge sphere far outside but reaching in: squares near 2^62 summed without overflow
        const int32_t big[3] = {2147483647, 0, 0}, c0[3] = {-2147483647 + 20, 8, 8}, c1[3] = {-2147483647 - 1, 8, 8};
        CHECK(edit_prepare(1, 1, c0, big, 16, 16, 16, d, noop) == 0 && !noop && d.hi[0] == 15);
        CHECK(edit_covers(d, 15, 8, 8) && edit_covers(d, 0, 0, 0));
        const int32_t c2[3] = {-2147483647 + 15, 8, 8};  // the ball ends at x = 15 on its axis only
        CHECK(edit_prepare(1, 1, c2, big, 16, 16, 16, d, noop) == 0 && !noop && edit_covers(d, 15, 8, 8) && !edit_covers(d, 15, 9, 8));
        CHECK(edit_prepare(1, 1, c1, big, 16, 16, 16, d, noop) == 0 && noop);  // box ends at x = -1
    }
    printf("plan: failures %d\n", fails);
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "plan";
    if (mode[0] == 'p') {
        check_plan();
    } else {
        const int f = argc > 2 ? atoi(argv[2]) : 8, S = argc > 3 ? atoi(argv[3]) : 64, rounds = argc > 4 ? atoi(argv[4]) : 20;
        check_bricks(f, S, rounds, 1234u + (unsigned)f);
    }
    printf("%s\n", fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
