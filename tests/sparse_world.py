"""Brickmap tables from a list of voxels, for grids too large for a dense array (1016 x 504 x 8 cells at f = 8 are 2.1 G
voxels): tables_from_voxels returns (coarse_bits, brick_slot, bounds, pool) in the oracle's layout, what
oracle/vxo_world.c:build_common and fill_brick make of the same voxels, ready for vxo.World.wrap and helpers.upload.

- cells in the reference's tiled order (vxo_sample_index64: 8x8x8 tiles stored linearly, tiles ordered x-fastest);
- slots in ascending tiled cell index;
- bounds of an empty cell (0, 0, 0, -1, -1, -1), of a non-empty one the inclusive brick-local extents as float;
- brick bits at the brick-local tiled index.

Every array is built once and without a Python loop over cells: the largest grid of tests/grid_shape_cases.py has 16.5 M
cells (396 MB of bounds, 66 MB of slots)."""
from __future__ import annotations

import numpy as np

EMPTY_SLOT = 0xFFFFFFFF


def tiled_index(x, y, z, width, height):
    """vxo_sample_index64 (oracle/vxo_trace.c) on int64 arrays"""
    tiles_w, tiles_h = width // 8, height // 8
    tile = (x >> 3) + (y >> 3) * tiles_w + (z >> 3) * (tiles_w * tiles_h)
    return tile * 512 + (x & 7) + (y & 7) * 8 + (z & 7) * 64


def tables_from_voxels(coords, cdims, factor):
    """coords: (n, 3) integer voxel coordinates (x, y, z) inside the grid, duplicates allowed; cdims: coarse cells per axis
    (multiples of 8); factor: brick edge (8, 16, 32)"""
    f = int(factor)
    cx, cy, cz = (int(c) for c in cdims)
    assert f in (8, 16, 32) and cx % 8 == 0 and cy % 8 == 0 and cz % 8 == 0 and min(cx, cy, cz) > 0
    ncells = cx * cy * cz
    bw = f ** 3 // 32
    p = np.asarray(coords, np.int64).reshape(-1, 3)
    assert (p >= 0).all() and (p < np.array([cx, cy, cz], np.int64) * f).all()
    cell, loc = p // f, p % f
    # one key per voxel, the cell's tiled index above the brick-local one: sorted, the voxels of a cell are adjacent, the
    # cells ascend (the slot order) and so do the bits of a brick
    key = np.unique(tiled_index(cell[:, 0], cell[:, 1], cell[:, 2], cx, cy) * f ** 3 + tiled_index(loc[:, 0], loc[:, 1], loc[:, 2], f, f))
    del p, cell, loc
    t, l = key // f ** 3, key % f ** 3
    first = np.flatnonzero(np.concatenate([[True], t[1:] != t[:-1]])) if len(t) else np.zeros(0, np.int64)
    cells = t[first]                       # the non-empty cells, ascending
    nslots = len(cells)
    brick_slot = np.full(ncells, EMPTY_SLOT, np.uint32)
    brick_slot[cells] = np.arange(nslots, dtype=np.uint32)
    flags = np.zeros(ncells, np.uint8)
    flags[cells] = 1
    coarse_bits = np.packbits(flags, bitorder="little").view(np.uint32).copy()
    del flags
    bounds = np.empty((ncells, 6), np.float32)
    bounds[:, :3] = 0.0
    bounds[:, 3:] = -1.0
    pool = np.zeros(nslots * bw, np.uint32)
    if nslots:
        # brick-local coordinates back from the brick-local tiled index
        tile, inside = l >> 9, l & 511
        tf = f // 8
        local = (((tile % tf) << 3) + (inside & 7), (((tile // tf) % tf) << 3) + ((inside >> 3) & 7), ((tile // (tf * tf)) << 3) + (inside >> 6))
        ext = np.empty((nslots, 6), np.float32)
        for a in range(3):
            ext[:, a] = np.minimum.reduceat(local[a], first)
            ext[:, 3 + a] = np.maximum.reduceat(local[a], first)
        bounds[cells] = ext
        # the pool: bit l of slot s is bit s * f^3 + l; the keys ascend, so the bits of a word are adjacent
        slot_of_voxel = np.cumsum(np.concatenate([[False], t[1:] != t[:-1]]))
        bit = slot_of_voxel * f ** 3 + l
        word = bit >> 5
        wfirst = np.flatnonzero(np.concatenate([[True], word[1:] != word[:-1]]))
        pool[word[wfirst]] = np.bitwise_or.reduceat(np.uint32(1) << (bit & 31).astype(np.uint32), wfirst)
    return coarse_bits, brick_slot, bounds, pool


def voxels_of_boxes(lo, size):
    """the voxels of solid boxes: lo (n, 3) lowest corners, size (n, 3) edge lengths; returns (m, 3) int64 coordinates"""
    lo, size = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(size, np.int64).reshape(-1, 3)
    vol = size.prod(1)
    owner = np.repeat(np.arange(len(lo)), vol)
    k = np.arange(vol.sum()) - np.repeat(np.cumsum(vol) - vol, vol)      # index of the voxel in its box
    sx, sy = size[owner, 0], size[owner, 1]
    return lo[owner] + np.stack([k % sx, (k // sx) % sy, k // (sx * sy)], 1)
