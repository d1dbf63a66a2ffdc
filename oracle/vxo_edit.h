/*
 * vxo_edit.h -- ORACLE (test infrastructure; parity unpinned, see vxo.h) of the voxel edits of this build's extension
 * include/vxrt.h vxrt_edit_voxels (the reference lists "Fully modifiable terrain" as to do, README.md:16).
 *
 * Ops have the layout of vxrt_edit_op.  BOX (kind 0): a <= v <= b on each axis; SPHERE (kind 1): dx^2 + dy^2 + dz^2 <= r^2
 * with d = v - a, r = b[0]; integers only, clipped to the world; the last op covering a voxel sets it to `value`.
 * vxo_apply_edits edits dense tiled-linear bits (the order of vxo_build_brickmap's input, VolumeRaytracer.cuh:107-131) in
 * place; it returns 0, or -1 and changes nothing on an invalid op: unknown kind, value not 0/1, negative radius, nonzero
 * b[1]/b[2] on a sphere.  Self-contained (built on its own into libvxo_edit.so by oracle/vxo_edit.py); the reference
 * for an edited world is vxo_build_brickmap of the edited grid.
 */
#ifndef VXO_EDIT_H
#define VXO_EDIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vxo_edit_op {
    int32_t kind, value;
    int32_t a[3], b[3];
} vxo_edit_op;

int vxo_apply_edits(uint32_t *dense_bits, int X, int Y, int Z, const vxo_edit_op *ops, size_t n);

#ifdef __cplusplus
}
#endif
#endif
