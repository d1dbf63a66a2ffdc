/*
 * vxo_edit.c -- ORACLE (test infrastructure; parity unpinned, see vxo.h): voxel edits on a dense tiled-linear grid.
 * Semantics in vxo_edit.h.
 */
#include "vxo_edit.h"

/* GetSampleIndex (VolumeRaytracer.cuh:107-131) with 64-bit arithmetic, as vxo_sample_index64 */
static uint64_t sample_index64(uint64_t x, uint64_t y, uint64_t z, uint64_t w, uint64_t h)
{
    const uint64_t tw = w / 8, th = h / 8;
    return ((x / 8) + (y / 8) * tw + (z / 8) * tw * th) * 512 + (x % 8) + (y % 8) * 8 + (z % 8) * 64;
}

int vxo_apply_edits(uint32_t *dense, int X, int Y, int Z, const vxo_edit_op *ops, size_t n)
{
    for (size_t k = 0; k < n; ++k) {
        const vxo_edit_op *o = &ops[k];
        if ((o->kind != 0 && o->kind != 1) || (o->value != 0 && o->value != 1))
            return -1;
        if (o->kind == 1 && (o->b[0] < 0 || o->b[1] != 0 || o->b[2] != 0))
            return -1;
    }
    const int64_t dim[3] = {X, Y, Z};
    for (size_t k = 0; k < n; ++k) {
        const vxo_edit_op *o = &ops[k];
        int64_t lo[3], hi[3];
        int empty = 0;
        for (int a = 0; a < 3; ++a) {
            lo[a] = o->kind == 0 ? (int64_t)o->a[a] : (int64_t)o->a[a] - o->b[0];
            hi[a] = o->kind == 0 ? (int64_t)o->b[a] : (int64_t)o->a[a] + o->b[0];
            if (lo[a] < 0)
                lo[a] = 0;
            if (hi[a] > dim[a] - 1)
                hi[a] = dim[a] - 1;
            if (lo[a] > hi[a])
                empty = 1;
        }
        if (empty)
            continue;
        /* inside the clipped box every |d| <= r < 2^31: the sum of squares is exact in uint64 */
        const uint64_t r2 = o->kind == 1 ? (uint64_t)o->b[0] * (uint64_t)o->b[0] : 0;
        for (int64_t z = lo[2]; z <= hi[2]; ++z)
            for (int64_t y = lo[1]; y <= hi[1]; ++y)
                for (int64_t x = lo[0]; x <= hi[0]; ++x) {
                    if (o->kind == 1) {
                        const int64_t dx = x - o->a[0], dy = y - o->a[1], dz = z - o->a[2];
                        if ((uint64_t)(dx * dx) + (uint64_t)(dy * dy) + (uint64_t)(dz * dz) > r2)
                            continue;
                    }
                    const uint64_t i = sample_index64((uint64_t)x, (uint64_t)y, (uint64_t)z, (uint64_t)X, (uint64_t)Y);
                    if (o->value)
                        dense[i >> 5] |= 1u << (i & 31);
                    else
                        dense[i >> 5] &= ~(1u << (i & 31));
                }
    }
    return 0;
}
