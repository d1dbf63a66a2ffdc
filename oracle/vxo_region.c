/*
 * vxo_region.c -- ORACLE (test infrastructure; parity unpinned, see vxo.h): region readback and voxel stamps on a dense
 * tiled-linear grid, one voxel at a time.  Semantics in vxo_region.h.
 */
#include "vxo_region.h"

/* GetSampleIndex (VolumeRaytracer.cuh:107-131) with 64-bit arithmetic, as vxo_sample_index64 */
static uint64_t sample_index64(uint64_t x, uint64_t y, uint64_t z, uint64_t w, uint64_t h)
{
    const uint64_t tw = w / 8, th = h / 8;
    return ((x / 8) + (y / 8) * tw + (z / 8) * tw * th) * 512 + (x % 8) + (y % 8) * 8 + (z % 8) * 64;
}

uint64_t vxo_region_words(const int32_t dims[3])
{
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1)
        return 0;
    const uint64_t limit = (uint64_t)1 << 36;
    const uint64_t v01 = (uint64_t)dims[0] * (uint64_t)dims[1];
    if (v01 > limit || (uint64_t)dims[2] > limit / v01)
        return 0;
    return ((uint64_t)dims[0] + 31) / 32 * (uint64_t)dims[1] * (uint64_t)dims[2];
}

/* bit index of region voxel (x, y, z) */
static uint64_t region_bit(const int32_t dims[3], uint64_t x, uint64_t y, uint64_t z)
{
    const uint64_t wpr = ((uint64_t)dims[0] + 31) / 32;
    return ((y + (uint64_t)dims[1] * z) * wpr + x / 32) * 32 + x % 32;
}

int vxo_read_region(const uint32_t *dense, int X, int Y, int Z, const int32_t o[3], const int32_t d[3], uint32_t *out)
{
    const uint64_t words = vxo_region_words(d);
    if (!words)
        return -1;
    for (uint64_t i = 0; i < words; ++i)
        out[i] = 0;
    const int64_t dim[3] = {X, Y, Z};
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = o[a] < 0 ? 0 : o[a];
        hi[a] = (int64_t)o[a] + d[a] - 1;
        if (hi[a] > dim[a] - 1)
            hi[a] = dim[a] - 1;
        if (lo[a] > hi[a])
            return 0;
    }
    for (int64_t z = lo[2]; z <= hi[2]; ++z)
        for (int64_t y = lo[1]; y <= hi[1]; ++y)
            for (int64_t x = lo[0]; x <= hi[0]; ++x) {
                const uint64_t i = sample_index64((uint64_t)x, (uint64_t)y, (uint64_t)z, (uint64_t)X, (uint64_t)Y);
                if ((dense[i >> 5] >> (i & 31)) & 1u) {
                    const uint64_t b = region_bit(d, (uint64_t)(x - o[0]), (uint64_t)(y - o[1]), (uint64_t)(z - o[2]));
                    out[b >> 5] |= 1u << (b & 31);
                }
            }
    return 0;
}

int vxo_apply_stamps(uint32_t *dense, int X, int Y, int Z, const vxo_stamp *stamps, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        const vxo_stamp *s = &stamps[k];
        if (!s->bits || s->mode < 0 || s->mode > 2 || s->reserved != 0 || !vxo_region_words(s->dims))
            return -1;
    }
    const int64_t dim[3] = {X, Y, Z};
    for (size_t k = 0; k < n; ++k) {
        const vxo_stamp *s = &stamps[k];
        int64_t lo[3], hi[3];
        int empty = 0;
        for (int a = 0; a < 3; ++a) {
            lo[a] = s->origin[a] < 0 ? 0 : s->origin[a];
            hi[a] = (int64_t)s->origin[a] + s->dims[a] - 1;
            if (hi[a] > dim[a] - 1)
                hi[a] = dim[a] - 1;
            if (lo[a] > hi[a])
                empty = 1;
        }
        if (empty)
            continue;
        for (int64_t z = lo[2]; z <= hi[2]; ++z)
            for (int64_t y = lo[1]; y <= hi[1]; ++y)
                for (int64_t x = lo[0]; x <= hi[0]; ++x) {
                    const uint64_t b = region_bit(s->dims, (uint64_t)(x - s->origin[0]), (uint64_t)(y - s->origin[1]),
                                                  (uint64_t)(z - s->origin[2]));
                    const int m = (int)((s->bits[b >> 5] >> (b & 31)) & 1u);
                    const uint64_t i = sample_index64((uint64_t)x, (uint64_t)y, (uint64_t)z, (uint64_t)X, (uint64_t)Y);
                    if (s->mode == 0 ? m : (s->mode == 1 && m))
                        dense[i >> 5] |= 1u << (i & 31);
                    else if (s->mode == 0 || m)
                        dense[i >> 5] &= ~(1u << (i & 31));
                }
    }
    return 0;
}
