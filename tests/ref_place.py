"""Two restatements of the voxel piece query (include/vxrt.h, vxrt_place_pieces) on dense bool [x, y, z] grids, and one of the
falling-island rule built on it (Context.drop_islands, VoxelRaytracer3D::DropIslands):
  place_shift      shifts the piece step by step and counts ov(j) by slicing;
  place_clearance  computes every voxel's clearance along the axis (the free steps before the next solid voxel) with
                   cumulative minima and takes the least over the piece's voxels; contact = the voxels with that clearance.
Both return (overlap, travel, contact, flags) for one placement; `place` runs a batch through one of them.
  drop_islands     the sequential rule on a dense world, with tests/ref_islands.py for the islands.
TEST INFRASTRUCTURE ONLY: imported by tests/ alone."""
from __future__ import annotations

import numpy as np

from tests import ref_islands as RI

MAX_PIECES, MAX_DIM, MAX_VOXELS, MAX_DIST, MAX_COORD = 64, 1024, 1 << 24, 4096, 1 << 30
BLOCKED, INVALID = 1, 2


def window(vox: np.ndarray, lo, dims) -> np.ndarray:
    """the voxels of the box lo .. lo + dims - 1, voxels outside the world empty"""
    out = np.zeros(tuple(int(d) for d in dims), bool)
    src, dst = [], []
    for k in range(3):
        a, b = max(int(lo[k]), 0), min(int(lo[k]) + int(dims[k]), vox.shape[k])
        if a >= b:
            return out
        src.append(slice(a, b))
        dst.append(slice(a - int(lo[k]), b - int(lo[k])))
    out[tuple(dst)] = vox[tuple(src)]
    return out


def valid(pl, n_pieces: int) -> bool:
    piece, ox, oy, oz, axis, dist = (int(v) for v in pl)
    return 0 <= piece < n_pieces and axis in (0, 1, 2) and abs(dist) <= MAX_DIST and all(abs(o) <= MAX_COORD for o in (ox, oy, oz))


def _ov(vox, piece, o) -> int:
    return int(np.count_nonzero(piece & window(vox, o, piece.shape)))


def place_shift(vox, piece, origin, axis: int, dist: int):
    piece = np.asarray(piece, bool)
    o = [int(v) for v in origin]
    s = 1 if dist > 0 else -1
    overlap = _ov(vox, piece, o)
    k = 0
    for j in range(1, abs(dist) + 1):
        oj = list(o)
        oj[axis] += s * j
        c = _ov(vox, piece, oj)
        if c:
            return overlap, s * k, c, BLOCKED
        k = j
    return overlap, s * k, 0, 0


def place_clearance(vox, piece, origin, axis: int, dist: int):
    piece = np.asarray(piece, bool)
    o = [int(v) for v in origin]
    ad = abs(int(dist))
    lo, dims = list(o), list(piece.shape)
    lo[axis] -= ad
    dims[axis] += 2 * ad
    w = np.moveaxis(window(vox, lo, dims), axis, 0)  # the piece's box and everything it sweeps; axis first
    p = np.moveaxis(piece, axis, 0)
    n = w.shape[0]
    here = w[ad: ad + p.shape[0]]
    overlap = int(np.count_nonzero(p & here))
    if ad == 0 or not p.any():
        return overlap, int(dist), 0, 0
    if dist < 0:  # look the other way: the same rule on the mirrored axis
        w, p = w[::-1], p[::-1]
    idx = np.arange(n, dtype=np.int64).reshape(-1, 1, 1)
    big = np.int64(1) << 40
    solid_at = np.where(w, idx, big)
    ahead = np.full(w.shape, big)  # index of the nearest solid voxel strictly ahead
    ahead[:-1] = np.minimum.accumulate(solid_at[::-1], axis=0)[::-1][1:]
    clear = (ahead - idx - 1)[ad: ad + p.shape[0]]
    least = int(clear[p].min())
    if least >= ad:
        return overlap, int(dist), 0, 0
    contact = int(np.count_nonzero(clear[p] == least))
    return overlap, (1 if dist > 0 else -1) * least, contact, BLOCKED


def place(vox, pieces, placements, how=place_clearance) -> np.ndarray:
    """a batch: (n, 4) int64 rows overlap, travel, contact, flags"""
    pl = np.asarray(placements, np.int64).reshape(-1, 6)
    out = np.zeros((len(pl), 4), np.int64)
    for i, r in enumerate(pl):
        if not valid(r, len(pieces)):
            out[i] = (0, 0, 0, INVALID)
        else:
            out[i] = how(vox, pieces[int(r[0])], r[1:4], int(r[4]), int(r[5]))
    return out


def pack_results(rows) -> np.ndarray:
    """(n, 4) rows as the uint32 words of vxrt_placed (travel as its two's complement)"""
    return np.asarray(rows, np.int64).astype(np.int32).view(np.uint32).reshape(-1, 4)


def drop_islands(vox, origin, dims, anchors: int = RI.FACES | RI.FLOOR, max_islands: int = 4096, how=place_clearance):
    """The falling-island rule on a dense world: returns (the world after, rows (id, voxels, travel, contact) in the order the
    islands were dropped).  Raises ValueError, with nothing changed, when the island table would be cut short or an island's
    box exceeds the piece limits."""
    origin = tuple(int(v) for v in origin)
    r = RI.fast(window(vox, origin, dims), origin, anchors)
    table = r["table"]
    if r["summary"][1] > max_islands:
        raise ValueError("island table cut short")
    for row in table:
        ext = row[5:8] - row[2:5]
        if ext.max() > MAX_DIM or int(ext.prod()) > MAX_VOXELS:
            raise ValueError("island beyond the piece limits")
    world = np.array(vox, bool)
    box = tuple(slice(max(origin[k], 0), max(min(origin[k] + int(dims[k]), vox.shape[k]), 0)) for k in range(3))
    inside = tuple(slice(box[k].start - origin[k], box[k].stop - origin[k]) for k in range(3))
    world[box] &= ~r["floating"][inside]
    rows = []
    for row in sorted(table.tolist(), key=lambda t: (t[3], t[0])):
        lo, hi = row[2:5], row[5:8]
        rel = tuple(slice(lo[k] - origin[k], hi[k] - origin[k]) for k in range(3))
        piece = r["labels"][rel] == row[0]
        _, travel, contact, _ = how(world, piece, lo, 1, -min(lo[1], MAX_DIST))
        at = (lo[0], lo[1] + travel, lo[2])
        src, dst = [], []
        for k in range(3):  # the union stamp, clipped to the world
            a, b = max(at[k], 0), min(at[k] + piece.shape[k], world.shape[k])
            src.append(slice(a - at[k], max(b - at[k], a - at[k])))
            dst.append(slice(a, max(b, a)))
        world[tuple(dst)] |= piece[tuple(src)]
        rows.append((row[0], row[1], travel, contact))
    return world, np.asarray(rows, np.int64).reshape(-1, 4)
