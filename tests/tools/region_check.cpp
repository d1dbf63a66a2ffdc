// Host harness of the region readback and stamp logic (voxelengine_amd/csrc/vxrt_region.hpp: the 32-voxel row gather of
// k_read_region, the stamp filter, the funnel-shifted gather of a stamp's bits and the per-row stamp step of
// k_stamp_bricks, stamp validation), compiled for the CPU through tests/tools/hoststub and compared with the oracle
// (oracle/vxo_region.c: vxo_read_region, vxo_apply_stamps; oracle/vxo_world.c: the brickmap builder).  Run by
// tests/test_region_host.py and, box by box, by tests/test_read_limits_host.py.
// build: g++ -O1 -std=c++17 -Itests/tools/hoststub -Ioracle tests/tools/region_check.cpp -x c oracle/vxo_*.c -lm -lpthread
#include "../../voxelengine_amd/csrc/vxrt_device.hpp"
#include "../../voxelengine_amd/csrc/vxrt_edit.hpp"
#include "../../voxelengine_amd/csrc/vxrt_region.hpp"
extern "C" {
#include "vxo.h"
#include "vxo_region.h"
}
#include "hbm_world.h"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace vxrt;

// what k_stamp_bricks computes for the brick at cell (bx, by, bz): the filter, one word of rows per lane, the extents
static void stamp_brick_host(const std::vector<StampDev>& st, const std::vector<uint32_t>& old, int bx, int by, int bz, int f,
                             std::vector<uint32_t>& img, uint32_t& ext, bool& changed)
{
    const int b0[3] = {bx * f, by * f, bz * f};
    size_t first = 0;
    for (size_t k = 0; k < st.size(); ++k)
        if (stamp_meets_brick(st[k], b0, f) && stamp_covers_brick(st[k], b0, f))
            first = k;
    std::vector<size_t> list;
    for (size_t k = first; k < st.size(); ++k)
        if (stamp_meets_brick(st[k], b0, f))
            list.push_back(k);
    const int lgf = brick_shift(f), rpw = 32 >> lgf;
    const uint32_t fmask = f == 32 ? 0xFFFFFFFFu : (1u << f) - 1u;
    img.assign(old.size(), 0u);
    int mn[2] = {0x7FFFFFFF, 0x7FFFFFFF}, mx[2] = {-1, -1};
    uint32_t xbits = 0u;
    for (uint32_t w = 0; w < (uint32_t)old.size(); ++w) {
        for (int s = 0; s < rpw; ++s) {
            const uint32_t q = w * (uint32_t)rpw + (uint32_t)s;
            const int lz = (int)(q & (uint32_t)(f - 1)), ly = (int)(q >> lgf);
            uint32_t row = (old[w] >> (s * f)) & fmask;
            for (size_t k : list)
                row = stamp_row(st[k], b0, f, ly, lz, row);
            img[w] |= row << (s * f);
            if (row) {
                xbits |= row;
                mn[0] = std::min(mn[0], ly); mn[1] = std::min(mn[1], lz);
                mx[0] = std::max(mx[0], ly); mx[1] = std::max(mx[1], lz);
            }
        }
    }
    ext = 0u;
    if (xbits) {
        const int emn[3] = {__builtin_ctz(xbits), mn[0], mn[1]}, emx[3] = {31 - __builtin_clz(xbits), mx[0], mx[1]};
        ext = edit_pack_extents(emn, emx);
    }
    changed = img != old;
}

static std::vector<uint32_t> random_dense(std::mt19937& rng, int X, int Y, int Z, double dens)
{
    std::vector<uint32_t> dense((size_t)X * Y * Z / 32, 0u);
    const uint32_t t = (uint32_t)(dens * 1000);
    for (int z = 0; z < Z; ++z) for (int y = 0; y < Y; ++y) for (int x = 0; x < X; ++x)
        if ((rng() % 1000) < t) vxo_bit_set(dense.data(), vxo_sample_index64(x, y, z, X, Y), 1);
    return dense;
}

static void random_box(std::mt19937& rng, const int dim[3], int32_t o[3], int32_t d[3], int maxd)
{
    for (int a = 0; a < 3; ++a) {
        const int span = std::min(dim[a], maxd);
        o[a] = (int)(rng() % (dim[a] + 2 * 40)) - 40;
        d[a] = 1 + (int)(rng() % (span + 20));
    }
    if (rng() % 6 == 0) d[0] = 1 + (int)(rng() % 3) * 32 + (int)(rng() % 2) - (int)(rng() % 2) * 2;  // 1, 31..33, 63..65
    if (d[0] < 1) d[0] = 1;
}

// reads: region_row_word (clipped as k_read_region clips) against vxo_read_region, random boxes on random worlds
static void check_read(int f, int X, int Y, int Z, int rounds, unsigned seed)
{
    std::mt19937 rng(seed);
    const int dim[3] = {X, Y, Z};
    size_t words = 0, set = 0;
    for (int r = 0; r < rounds; ++r) {
        std::vector<uint32_t> dense = random_dense(rng, X, Y, Z, 0.05 + 0.3 * (r % 3));
        vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
        const HbmWorld h = to_hbm(w);
        for (int q = 0; q < 24; ++q) {
            int32_t o[3], d[3];
            random_box(rng, dim, o, d, 96);
            if (q == 0) { o[0] = -5; o[1] = -7; o[2] = -9; d[0] = X + 10; d[1] = std::min(Y + 14, 40); d[2] = 3; }  // every face
            if (q == 1) { o[0] = X; o[1] = 0; o[2] = 0; d[0] = 40; d[1] = 3; d[2] = 3; }                           // wholly outside
            if (q == 2) { o[0] = X / 2; o[1] = Y / 2; o[2] = Z / 2; d[0] = d[1] = d[2] = 1; }                    // one voxel
            const std::vector<uint32_t> got = read_host(h.world(), o, d);
            std::vector<uint32_t> want(got.size(), 0u);
            CHECK(vxo_read_region(dense.data(), X, Y, Z, o, d, want.data()) == 0);
            CHECK(got == want);
            words += got.size();
            for (uint32_t v : got) set += __builtin_popcount(v);
        }
        vxo_world_free(w);
    }
    printf("read f=%d %dx%dx%d: %zu words checked, %zu voxels set, failures %d\n", f, X, Y, Z, words, set, fails);
}

// one given box on a random world (tests/test_read_limits_host.py: the boxes of tests/read_limit_cases.py)
static void check_box(int f, int X, int Y, int Z, const int32_t o[3], const int32_t d[3], unsigned seed)
{
    std::mt19937 rng(seed);
    std::vector<uint32_t> dense = random_dense(rng, X, Y, Z, 0.4);
    vxo_world* w = vxo_build_brickmap(dense.data(), X, Y, Z, f);
    const HbmWorld h = to_hbm(w);
    const std::vector<uint32_t> got = read_host(h.world(), o, d);
    std::vector<uint32_t> want(got.size(), 0u);
    CHECK(got.size() == region_words(d));
    CHECK(vxo_read_region(dense.data(), X, Y, Z, o, d, want.data()) == 0);
    CHECK(got == want);
    size_t set = 0;
    for (uint32_t v : got) set += __builtin_popcount(v);
    vxo_world_free(w);
    printf("box f=%d %dx%dx%d at %d %d %d of %d %d %d: %zu words checked, %zu voxels set, failures %d\n", f, X, Y, Z, o[0], o[1], o[2],
           d[0], d[1], d[2], got.size(), set, fails);
}

// stamps: the per-brick logic against the oracle's rebuilt brickmap of the stamped dense grid, every brick of the world
static void check_stamps(int f, int X, int Y, int Z, int rounds, unsigned seed)
{
    std::mt19937 rng(seed);
    const int dim[3] = {X, Y, Z}, cx = X / f, cy = Y / f, cz = Z / f;
    size_t bricks = 0, changed_total = 0;
    for (int r = 0; r < rounds; ++r) {
        std::vector<uint32_t> dense = random_dense(rng, X, Y, Z, 0.1 * (r % 3));
        const int nst = 1 + (int)(rng() % 8);
        std::vector<std::vector<uint32_t>> bits((size_t)nst);
        std::vector<vxo_stamp> os;
        std::vector<StampDev> dev;
        for (int k = 0; k < nst; ++k) {
            vxo_stamp s{};
            random_box(rng, dim, s.origin, s.dims, X / 2 + 8);
            if (rng() % 5 == 0)  // a replace stamp over the whole world: later stamps only matter
                for (int a = 0; a < 3; ++a) { s.origin[a] = -3; s.dims[a] = dim[a] + 6; }
            s.mode = (int)(rng() % 3);
            const double dens = (rng() % 4) * 0.3;
            bits[k].assign(region_words(s.dims), 0u);
            for (uint32_t& v : bits[k]) {
                v = 0u;
                for (int b = 0; b < 32; ++b)
                    if ((rng() % 100) < dens * 100) v |= 1u << b;
            }
            s.bits = bits[k].data();
            os.push_back(s);
            StampDev d;
            bool noop = false;
            CHECK(stamp_prepare(s.bits, s.origin, s.dims, s.mode, 0, X, Y, Z, d, noop) == 0);
            if (!noop)
                dev.push_back(d);
        }
        vxo_world* before = vxo_build_brickmap(dense.data(), X, Y, Z, f);
        std::vector<uint32_t> stamped = dense;
        CHECK(vxo_apply_stamps(stamped.data(), X, Y, Z, os.data(), os.size()) == 0);
        vxo_world* after = vxo_build_brickmap(stamped.data(), X, Y, Z, f);
        for (int bz = 0; bz < cz; ++bz) for (int by = 0; by < cy; ++by) for (int bx = 0; bx < cx; ++bx) {
            const uint32_t t = ref_tiled_index(bx, by, bz, cx / 8, cy / 8);
            std::vector<uint32_t> img;
            uint32_t ext = 0;
            bool changed = false;
            stamp_brick_host(dev, hbm_brick(before, before->brick_slot[t], f), bx, by, bz, f, img, ext, changed);
            uint32_t want_ext = 0;
            if (after->brick_slot[t] != VXO_EMPTY_SLOT)
                for (int k = 0; k < 6; ++k) want_ext |= (uint32_t)(int)after->bounds[t * 6 + k] << (5 * k);
            CHECK(img == hbm_brick(after, after->brick_slot[t], f));
            CHECK(ext == want_ext);
            ++bricks;
            changed_total += changed;
        }
        vxo_world_free(before);
        vxo_world_free(after);
    }
    printf("stamps f=%d %dx%dx%d: %zu bricks checked, %zu changed, failures %d\n", f, X, Y, Z, bricks, changed_total, fails);
}

// hand-derived cases of the helpers, and validation
static void check_units()
{
    const uint32_t row[3] = {0x80000001u, 0x00000003u, 0xFFFFFFFFu};
    CHECK(row_gather32(row, 3, 0) == 0x80000001u);
    CHECK(row_gather32(row, 3, 31) == 0x00000007u);        // bit 31 of word 0, then bits 0, 1 of word 1
    CHECK(row_gather32(row, 3, -1) == 0x00000002u);        // the word before the row reads 0
    CHECK(row_gather32(row, 3, 64) == 0xFFFFFFFFu && row_gather32(row, 3, 65) == 0x7FFFFFFFu);  // past the row: 0
    CHECK(row_gather32(row, 3, -40) == 0u && row_gather32(row, 3, 96) == 0u);
    CHECK(bit_range(0, 31) == 0xFFFFFFFFu && bit_range(3, 3) == 8u && bit_range(4, 7) == 0xF0u);
    CHECK(place_bits(0xFFu, 0) == 0xFFu && place_bits(0xFFu, 28) == 0xF0000000u && place_bits(0xFFu, -4) == 0x0Fu);
    CHECK(place_bits(1u, 31) == 0x80000000u && place_bits(0x80000000u, -31) == 1u);
    const int32_t one[3] = {1, 1, 1}, big[3] = {1 << 12, 1 << 12, 1 << 12}, over[3] = {1 << 12, 1 << 12, (1 << 12) + 1};
    const int32_t zero[3] = {0, 5, 5}, neg[3] = {4, -1, 4}, w33[3] = {33, 2, 3};
    CHECK(region_words(one) == 1 && region_words(big) == (1ull << 31) && region_words(over) == 0);
    CHECK(region_words(zero) == 0 && region_words(neg) == 0 && region_words(w33) == 12);
    const int32_t huge[3] = {2147483647, 2147483647, 2147483647};
    CHECK(region_words(huge) == 0);
    StampDev d;
    bool noop;
    const uint32_t b = 0;
    const int32_t o[3] = {0, 0, 0}, dd[3] = {4, 4, 4};
    CHECK(stamp_prepare(&b, o, dd, 3, 0, 16, 16, 16, d, noop) != 0);
    CHECK(stamp_prepare(&b, o, dd, -1, 0, 16, 16, 16, d, noop) != 0);
    CHECK(stamp_prepare(&b, o, dd, 0, 1, 16, 16, 16, d, noop) != 0);
    CHECK(stamp_prepare(nullptr, o, dd, 0, 0, 16, 16, 16, d, noop) != 0);
    CHECK(stamp_prepare(&b, o, zero, 0, 0, 16, 16, 16, d, noop) != 0);
    CHECK(stamp_prepare(&b, o, over, 1, 0, 16, 16, 16, d, noop) != 0);
    CHECK(stamp_prepare(&b, o, dd, 2, 0, 16, 16, 16, d, noop) == 0 && !noop && d.wpr == 1 && d.hi[0] == 3);
    const int32_t far[3] = {2147483647, 0, 0}, farneg[3] = {-2147483647 - 1, 0, 0}, long_[3] = {2147483647, 1, 1};
    CHECK(stamp_prepare(&b, far, dd, 0, 0, 16, 16, 16, d, noop) == 0 && noop);
    CHECK(stamp_prepare(&b, farneg, long_, 0, 0, 16, 16, 16, d, noop) == 0 && noop);  // ends at x = -2
    const int32_t reach[3] = {-2147483647 + 10, 0, 0};
    CHECK(stamp_prepare(&b, reach, long_, 0, 0, 16, 16, 16, d, noop) == 0 && !noop && d.lo[0] == 0 && d.hi[0] == 9);
    printf("units: failures %d\n", fails);
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "units";
    if (mode[0] == 'u') {
        check_units();
    } else {
        const int f = argc > 2 ? atoi(argv[2]) : 8, X = argc > 3 ? atoi(argv[3]) : 64, Y = argc > 4 ? atoi(argv[4]) : X,
                  Z = argc > 5 ? atoi(argv[5]) : X, rounds = argc > 6 ? atoi(argv[6]) : 4;
        if (mode[0] == 'b' && argc > 11) {  // box f X Y Z ox oy oz dx dy dz
            const int32_t o[3] = {atoi(argv[6]), atoi(argv[7]), atoi(argv[8])}, d[3] = {atoi(argv[9]), atoi(argv[10]), atoi(argv[11])};
            check_box(f, X, Y, Z, o, d, 2468u + (unsigned)f);
        } else if (mode[0] == 'r')
            check_read(f, X, Y, Z, rounds, 4321u + (unsigned)f);
        else
            check_stamps(f, X, Y, Z, rounds, 8765u + (unsigned)f);
    }
    printf("%s\n", fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
