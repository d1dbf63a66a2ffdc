"""Restatements of the stamp orientations (include/vxrt.h, vxrt_orientation / vxrt_transform_stamp) on bool [x, y, z] numpy
grids, written from the header's rule alone: an orientation is (axis, flip); destination axis k runs along source axis
axis[k], against it when bit k of flip is set; dd[k] = sd[axis[k]]; source voxel p lands at q with
q[k] = sd[axis[k]] - 1 - p[axis[k]] if flip bit k else p[axis[k]].

  transform        np.transpose plus np.flip
  transform_loop   one voxel at a time with the index rule
  summary          (voxels, set_min, set_max) of a grid, the sentinels for an empty one
  pack_padded      region words of a grid with the padding bits at the end of every row SET (a transform must ignore them)
"""
import itertools

import numpy as np

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
IDENTITY = ((0, 1, 2), 0)


def all_orientations():
    """the 48 (axis, flip) pairs"""
    return [(axis, flip) for axis in itertools.permutations((0, 1, 2)) for flip in range(8)]


def dims(o, sd):
    return tuple(int(sd[a]) for a in o[0])


def voxel(o, sd, p):
    axis, flip = o
    return tuple(sd[axis[k]] - 1 - p[axis[k]] if (flip >> k) & 1 else p[axis[k]] for k in range(3))


def transform(grid, o):
    axis, flip = o
    out = np.transpose(np.asarray(grid, bool), axis)
    for k in range(3):
        if (flip >> k) & 1:
            out = np.flip(out, k)
    return np.ascontiguousarray(out)


def transform_loop(grid, o):
    g = np.asarray(grid, bool)
    out = np.zeros(dims(o, g.shape), bool)
    for p in np.ndindex(*g.shape):
        out[voxel(o, g.shape, p)] = g[p]
    return out


def is_rotation(o):
    """the determinant of the signed permutation matrix is +1"""
    axis, flip = o
    m = np.zeros((3, 3), int)
    for k in range(3):
        m[k, axis[k]] = -1 if (flip >> k) & 1 else 1
    return round(float(np.linalg.det(m))) == 1


def compose(a, b):
    """a first, then b, by the header's formula"""
    axis = tuple(a[0][b[0][k]] for k in range(3))
    flip = sum((((b[1] >> k) ^ (a[1] >> b[0][k])) & 1) << k for k in range(3))
    return axis, flip


def rotation(axis, turns):
    """right-handed quarter turns about `axis`: one takes axis a + 1 onto a + 2, i.e. q[a + 2] = p[a + 1],
    q[a + 1] = sd[a + 2] - 1 - p[a + 2]"""
    b, c = (axis + 1) % 3, (axis + 2) % 3
    ax = [0, 0, 0]
    ax[axis], ax[b], ax[c] = axis, c, b
    one, out = (tuple(ax), 1 << b), IDENTITY
    for _ in range(turns % 4):
        out = compose(out, one)
    return out


def summary(grid):
    g = np.asarray(grid, bool)
    idx = np.argwhere(g)
    if len(idx) == 0:
        return 0, (INT32_MAX,) * 3, (INT32_MIN,) * 3
    return len(idx), tuple(int(v) for v in idx.min(0)), tuple(int(v) for v in idx.max(0))


def pack(grid):
    """bool [x, y, z] -> region words, padding bits 0"""
    v = np.asarray(grid, bool)
    X, Y, Z = v.shape
    rows = np.zeros((Z, Y, (X + 31) // 32 * 32), bool)
    rows[:, :, :X] = v.transpose(2, 1, 0)
    return np.packbits(rows, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


def pack_padded(grid):
    """the same with every padding bit at the end of a row set"""
    v = np.asarray(grid, bool)
    X, Y, Z = v.shape
    rows = np.ones((Z, Y, (X + 31) // 32 * 32), bool)
    rows[:, :, :X] = v.transpose(2, 1, 0)
    return np.packbits(rows, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


def unpack(words, d):
    """region words -> (bool [x, y, z], the padding bits as a bool array)"""
    X, Y, Z = (int(v) for v in d)
    wpr = (X + 31) // 32
    w = np.ascontiguousarray(words).view(np.uint32)[: wpr * Y * Z].reshape(Z, Y, wpr)
    bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")
    return bits[:, :, :X].astype(bool).transpose(2, 1, 0), bits[:, :, X:].astype(bool)


def crop(grid):
    """the grid cut to the bounding box of its set voxels"""
    n, lo, hi = summary(grid)
    assert n
    return np.asarray(grid, bool)[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
