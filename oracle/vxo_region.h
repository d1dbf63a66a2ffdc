/*
 * vxo_region.h -- ORACLE (test infrastructure; parity unpinned, see vxo.h) of the region readback and voxel stamps of this
 * build's extension include/vxrt.h vxrt_read_region / vxrt_edit_stamps.
 *
 * Region layout: a box of dims[0] x dims[1] x dims[2] voxels whose voxel (0,0,0) is world voxel origin; row (y, z) is
 * ceil(dims[0] / 32) 32-bit words, rows y fastest, then z: voxel (x, y, z) is bit (x & 31) of word
 * (y + dims[1] * z) * ceil(dims[0] / 32) + (x >> 5).  Valid dims: each >= 1, at most 2^36 voxels in all.
 * vxo_read_region reads dense tiled-linear bits (the order of vxo_build_brickmap's input, VolumeRaytracer.cuh:107-131)
 * into a region: voxels outside the world and padding bits 0.  vxo_apply_stamps writes stamps into dense bits in place,
 * in order: with m the stamp's bit at v - origin, REPLACE (0) sets every voxel of the stamp's box to m, UNION (1) sets
 * the voxels with m = 1, SUBTRACT (2) clears the voxels with m = 1; clipped to the world.  Both return 0, or -1 and change
 * nothing on invalid input: bad dims, a NULL bits pointer, an unknown mode or nonzero reserved.  Self-contained (built on
 * its own into libvxo_region.so by oracle/vxo_region.py); the reference for a stamped world is vxo_build_brickmap of the
 * stamped grid.
 */
#ifndef VXO_REGION_H
#define VXO_REGION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vxo_stamp {
    const uint32_t *bits;
    int32_t origin[3];
    int32_t dims[3];
    int32_t mode;
    int32_t reserved;
} vxo_stamp;

uint64_t vxo_region_words(const int32_t dims[3]);
int vxo_read_region(const uint32_t *dense_bits, int X, int Y, int Z, const int32_t origin[3], const int32_t dims[3],
                    uint32_t *out);
int vxo_apply_stamps(uint32_t *dense_bits, int X, int Y, int Z, const vxo_stamp *stamps, size_t n);

#ifdef __cplusplus
}
#endif
#endif
