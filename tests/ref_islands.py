"""Two restatements of the floating-island contract (include/vxrt.h, vxrt_find_islands) on a bool [x, y, z] grid of the box:
  find_islands        pure numpy: min-label propagation over the six face neighbours with pointer jumping, then the anchor
                      and table rules;
  find_islands_scipy  scipy.ndimage.label with the 6-connected structure (used when scipy imports), the same rules.
Both return {"labels": uint32 [x, y, z] (0 empty, else the component id), "floating": bool [x, y, z], "table": rows
(id, voxels, lo[3], hi[3]) in ascending id as an (n, 8) int64 array, "summary": (components, islands, island_voxels)}.
TEST INFRASTRUCTURE ONLY: imported by tests/ alone."""
from __future__ import annotations

import numpy as np

X_LO, X_HI, Y_LO, Y_HI, Z_LO, Z_HI, FLOOR = 1, 2, 4, 8, 16, 32, 64
FACES = 63


def region_index(dims) -> np.ndarray:
    """x + dims[0] * (y + dims[1] * z) of every voxel, as an int64 [x, y, z] grid"""
    X, Y, Z = dims
    return np.arange(X * Y * Z, dtype=np.int64).reshape(Z, Y, X).transpose(2, 1, 0)


def anchor_mask(dims, origin, anchors: int) -> np.ndarray:
    """the anchor voxels of the box: on a set face, or at world y = 0 with FLOOR"""
    a = np.zeros(tuple(dims), bool)
    for k in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[k], hi[k] = 0, dims[k] - 1
        if anchors >> (2 * k) & 1:
            a[tuple(lo)] = True
        if anchors >> (2 * k + 1) & 1:
            a[tuple(hi)] = True
    if anchors & FLOOR and 0 <= -origin[1] < dims[1]:
        a[:, -origin[1], :] = True
    return a


def _min_labels(vox: np.ndarray) -> np.ndarray:
    """component id (min region index + 1) of every solid voxel, 0 for empty: propagation + pointer jumping"""
    dims = vox.shape
    idx = region_index(dims)
    big = np.int64(1) << 40
    lab = np.where(vox, idx + 1, big)
    while True:
        old = lab.copy()
        for k in range(3):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[k], b[k] = slice(1, None), slice(None, -1)
            a, b = tuple(a), tuple(b)
            both = vox[a] & vox[b]
            m = np.minimum(lab[a], lab[b])
            lab[a] = np.where(both, m, lab[a])
            lab[b] = np.where(both, np.minimum(lab[b], m), lab[b])
        # pointer jumping: a voxel takes the label of the voxel its label names, until that changes nothing
        flat = lab.transpose(2, 1, 0).reshape(-1)
        solid = flat < big
        while True:
            j = flat.copy()
            j[solid] = flat[flat[solid] - 1]
            if np.array_equal(j, flat):
                break
            flat = j
        lab = flat.reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0).copy()
        if np.array_equal(lab, old):
            break
    return np.where(vox, lab, 0).astype(np.int64)


def _scipy_labels(vox: np.ndarray) -> np.ndarray:
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, 1)  # six face neighbours
    lab, n = ndimage.label(vox, structure=st)
    if n == 0:
        return np.zeros(vox.shape, np.int64)
    idx = region_index(vox.shape)
    first = np.full(n + 1, np.int64(1) << 40)
    np.minimum.at(first, lab[vox], idx[vox])
    return np.where(vox, first[lab] + 1, 0).astype(np.int64)


def _rules(labels: np.ndarray, origin, anchors: int) -> dict:
    dims = labels.shape
    solid = labels > 0
    ids = np.unique(labels[solid])
    anchored = np.unique(labels[solid & anchor_mask(dims, origin, anchors)])
    island_ids = np.setdiff1d(ids, anchored)
    floating = solid & np.isin(labels, island_ids)
    rows = np.zeros((len(island_ids), 8), np.int64)
    if len(island_ids):
        g = np.nonzero(floating)
        lv = labels[g]
        k = np.searchsorted(island_ids, lv)
        rows[:, 0] = island_ids
        rows[:, 1] = np.bincount(k, minlength=len(island_ids))
        for a in range(3):
            c = g[a].astype(np.int64) + origin[a]
            lo = np.full(len(island_ids), np.iinfo(np.int64).max)
            hi = np.full(len(island_ids), np.iinfo(np.int64).min)
            np.minimum.at(lo, k, c)
            np.maximum.at(hi, k, c)
            rows[:, 2 + a], rows[:, 5 + a] = lo, hi + 1
    return {"labels": labels.astype(np.uint32), "floating": floating, "table": rows,
            "summary": (len(ids), len(island_ids), int(floating.sum()))}


def find_islands(vox: np.ndarray, origin=(0, 0, 0), anchors: int = FACES | FLOOR) -> dict:
    """the contract on the box's voxels ``vox`` (bool [x, y, z], voxels outside the world already empty)"""
    return _rules(_min_labels(np.asarray(vox, bool)), tuple(int(v) for v in origin), int(anchors))


def find_islands_scipy(vox: np.ndarray, origin=(0, 0, 0), anchors: int = FACES | FLOOR) -> dict:
    return _rules(_scipy_labels(np.asarray(vox, bool)), tuple(int(v) for v in origin), int(anchors))


def have_scipy() -> bool:
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except ImportError:
        return False


def fast(vox, origin=(0, 0, 0), anchors: int = FACES | FLOOR) -> dict:
    """scipy when it imports, else numpy: for the large grids of the GPU tests"""
    return (find_islands_scipy if have_scipy() else find_islands)(vox, origin, anchors)


def table_rows(table) -> np.ndarray:
    """an ISLAND_DTYPE table (or (n, 8) int array) as (n, 8) int64 rows, for comparisons"""
    t = np.asarray(table)
    if t.dtype.names:
        return np.column_stack([t["id"], t["voxels"], t["lo"], t["hi"]]).astype(np.int64).reshape(-1, 8)
    return t.astype(np.int64).reshape(-1, 8)


def snake(dims) -> np.ndarray:
    """a single 6-connected path that winds through the whole box: serpentine rows two voxels apart in x, y and z, joined at
    their ends, layers joined at alternating corners -- the worst case for label propagation depth"""
    X, Y, Z = dims
    v = np.zeros(dims, bool)
    ys = list(range(0, Y, 2))
    zs = list(range(0, Z, 2))
    for zi, z in enumerate(zs):
        order = ys if zi % 2 == 0 else ys[::-1]
        for ri, y in enumerate(order):
            v[:, y, z] = True
            if ri + 1 < len(order):  # join to the next row at alternating ends
                x = X - 1 if ri % 2 == 0 else 0
                y2 = order[ri + 1]
                v[x, min(y, y2):max(y, y2) + 1, z] = True
        if zi + 1 < len(zs):  # join to the next layer where this layer's last row ends
            last = order[-1]
            x = X - 1 if (len(order) - 1) % 2 == 0 else 0
            v[x, last, z:zs[zi + 1] + 1] = True
    return v
