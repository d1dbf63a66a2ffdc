"""A second, independent restatement of the region readback and voxel stamps (include/vxrt.h, vxrt_read_region /
vxrt_edit_stamps; C: oracle/vxo_region.c) in numpy, on a bool [x, y, z] grid, written with slices and zero padding so that
the two restatements can be held against each other.  Regions are bool [x, y, z] grids here; packing to the region words
is voxelengine_amd.pack_region / unpack_region.  TEST INFRASTRUCTURE ONLY (like the rest of oracle/): imported by tests/
alone."""
from __future__ import annotations

import numpy as np

REPLACE, UNION, SUBTRACT = 0, 1, 2


def _overlap(origin, dims, shape):
    """the world slice and the region slice of the box's part inside the world, or None"""
    w, r = [], []
    for o, d, n in zip(origin, dims, shape):
        lo, hi = max(int(o), 0), min(int(o) + int(d), n)
        if lo >= hi:
            return None
        w.append(slice(lo, hi))
        r.append(slice(lo - int(o), hi - int(o)))
    return tuple(w), tuple(r)


def read_region(vox: np.ndarray, origin, dims) -> np.ndarray:
    """bool [dims] grid of the box origin .. origin + dims - 1: the world's voxels, zero outside it"""
    out = np.zeros(tuple(int(d) for d in dims), bool)
    ov = _overlap(origin, dims, vox.shape)
    if ov is not None:
        out[ov[1]] = vox[ov[0]]
    return out


def apply_stamps(vox: np.ndarray, stamps) -> np.ndarray:
    """stamps: (origin, mask, mode) with mask a bool [x, y, z] grid; in order, the last stamp covering a voxel decides it.
    Returns the stamped copy; raises ValueError on an unknown mode (all stamps are checked before any change)."""
    out = np.array(vox, bool, copy=True)
    for _, mask, mode in stamps:
        if mode not in (REPLACE, UNION, SUBTRACT) or np.asarray(mask).ndim != 3 or 0 in np.asarray(mask).shape:
            raise ValueError("invalid stamp")
    for origin, mask, mode in stamps:
        mask = np.asarray(mask, bool)
        ov = _overlap(origin, mask.shape, out.shape)
        if ov is None:
            continue
        m = mask[ov[1]]
        if mode == REPLACE:
            out[ov[0]] = m
        elif mode == UNION:
            out[ov[0]] |= m
        else:
            out[ov[0]] &= ~m
    return out
