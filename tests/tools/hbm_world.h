// What the host harnesses of the world queries share (tests/tools/*_check.cpp): the failure counter and CHECK, the index
// recorder behind VXRT_ISL_CHECK / VXRT_NAV_CHECK, the oracle's brickmap (oracle/vxo_world.c) laid out as the library holds
// it in HBM, and the host emulation of k_read_region.  A harness that checks indices declares check_index and defines its
// VXRT_*_CHECK macro before it includes the library's headers.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../voxelengine_amd/csrc/vxrt_region.hpp"
extern "C" {
#include "vxo.h"
}

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            if (fails < 20)                                           \
                printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++fails;                                                  \
        }                                                             \
    } while (0)

// g_size[array]: the size of the array with that id (kIsl* / kNav*); every index the library code forms is checked against it
static uint64_t checked = 0;
static uint64_t g_size[32];
static inline void check_index(int array, uint64_t index)
{
    ++checked;
    if (index >= g_size[array]) {
        if (fails < 20)
            printf("FAIL: index %llu of array %d (size %llu)\n", (unsigned long long)index, array, (unsigned long long)g_size[array]);
        ++fails;
    }
}

// brick `slot` of an oracle world (tiled bits) in the HBM bit order of the library (x, z, y); zeros for an empty cell
static inline std::vector<uint32_t> hbm_brick(const vxo_world* w, uint32_t slot, int f)
{
    const uint32_t bw = f * f * f / 32;
    std::vector<uint32_t> out(bw, 0u);
    if (slot == VXO_EMPTY_SLOT)
        return out;
    for (int z = 0; z < f; ++z) for (int y = 0; y < f; ++y) for (int x = 0; x < f; ++x) {
        const uint32_t t = vxrt::ref_tiled_index(x, y, z, f / 8, f / 8), i = (uint32_t)vxrt::hbm_index(x, y, z, f, f);
        if ((w->pool[(size_t)slot * bw + (t >> 5)] >> (t & 31)) & 1u) out[i >> 5] |= 1u << (i & 31);
    }
    return out;
}

// an oracle world as the library holds it in HBM: cell records (slots) in HBM cell order, bricks in HBM bit order
struct HbmWorld {
    int f, cd[3];
    std::vector<uint2> meta;
    std::vector<uint32_t> pool;
    vxrt::CollideWorld world() const { return vxrt::query_world(meta.data(), pool.data(), f, cd); }
};

static inline HbmWorld to_hbm(const vxo_world* w)
{
    HbmWorld h;
    h.f = w->factor;
    const int cx = w->cdims[0], cy = w->cdims[1], cz = w->cdims[2];
    h.cd[0] = cx;
    h.cd[1] = cy;
    h.cd[2] = cz;
    h.meta.assign((size_t)w->ncells, make_uint2(vxrt::kEmptySlot, 0u));
    for (int bz = 0; bz < cz; ++bz) for (int by = 0; by < cy; ++by) for (int bx = 0; bx < cx; ++bx)
        h.meta[vxrt::hbm_index(bx, by, bz, cx, cz)].x = w->brick_slot[vxrt::ref_tiled_index(bx, by, bz, cx / 8, cy / 8)];
    for (uint64_t s = 0; s < w->nslots; ++s) {
        const std::vector<uint32_t> b = hbm_brick(w, (uint32_t)s, h.f);
        h.pool.insert(h.pool.end(), b.begin(), b.end());
    }
    return h;
}

// what k_read_region writes for the box o, d (region layout): each word clipped to the world before any load, then
// region_row_word and the pad mask of a row's last word
static inline std::vector<uint32_t> read_host(const vxrt::CollideWorld& W, const int32_t o[3], const int32_t d[3])
{
    const uint64_t wpr = vxrt::region_words_per_row(d[0]);
    std::vector<uint32_t> out(vxrt::region_words(d), 0xDEADBEEFu);
    for (int64_t zl = 0; zl < d[2]; ++zl) for (int64_t yl = 0; yl < d[1]; ++yl) for (uint64_t xw = 0; xw < wpr; ++xw) {
        const int64_t x0 = (int64_t)o[0] + 32 * (int64_t)xw, wy = (int64_t)o[1] + yl, wz = (int64_t)o[2] + zl;
        uint32_t w = 0u;
        if (wy >= 0 && wy < W.dim[1] && wz >= 0 && wz < W.dim[2] && x0 + 31 >= 0 && x0 < W.dim[0])
            w = vxrt::region_row_word(W.meta, W.pool, W.f, W.lgf, W.cx, W.cz, x0, (int)wy, (int)wz);
        out[((uint64_t)yl + (uint64_t)d[1] * zl) * wpr + xw] = w & (xw == wpr - 1 ? vxrt::row_last_mask(d[0]) : 0xFFFFFFFFu);
    }
    return out;
}
