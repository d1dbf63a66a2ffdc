"""Two independent restatements of surface extraction (include/vxrt.h, vxrt_extract_surface) on dense numpy grids.

``extract`` is the declarative definition, vectorised: the runs of every row of a mask by shifts, a quad start where the
row above does not hold the identical run, the height by counting the rows below that continue it.  ``extract_scan`` is a
plain scan, row by row, that keeps the set of open runs of the row above.  Both return a ``Surface``: the packed quads in
canonical order, the vertices and triangles of those quads, and the summary's 16 words.

A world is a bool [x, y, z] grid; voxels outside it are empty.  Directions d = 0 .. 5 are -x, +x, -y, +y, -z, +z.
"""
from typing import NamedTuple

import numpy as np

CAP, OPEN = 0, 1
# mask axes [s, v, u] as axes of the [x, y, z] grid: (y, z) for x, (x, z) for y, (x, y) for z
_SVU = {0: (0, 2, 1), 1: (1, 2, 0), 2: (2, 1, 0)}
_STEP = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]


class Surface(NamedTuple):
    quads: np.ndarray      # (n, 2) uint32: pos, ext
    vertices: np.ndarray   # (4 n, 3) int32
    triangles: np.ndarray  # (2 n, 3) uint32
    summary: np.ndarray    # 16 uint32: solid, faces, quads, written, faces_dir[6], quads_dir[6]

    def cut(self, capacity):
        """what a call with room for ``capacity`` quads writes, and its summary"""
        n = min(len(self.quads), int(capacity))
        s = self.summary.copy()
        s[3] = n
        return Surface(self.quads[:n], self.vertices[:4 * n], self.triangles[:2 * n], s)


def halo_box(world, origin, dims):
    """the box grown by one voxel on every side as a bool [x, y, z] grid, empty outside the world"""
    world = np.asarray(world, bool)
    out = np.zeros(tuple(int(d) + 2 for d in dims), bool)
    lo = [int(o) - 1 for o in origin]
    a = [max(l, 0) for l in lo]
    b = [min(l + n, w) for l, n, w in zip(lo, out.shape, world.shape)]
    if all(x < y for x, y in zip(a, b)):
        out[a[0] - lo[0]:b[0] - lo[0], a[1] - lo[1]:b[1] - lo[1], a[2] - lo[2]:b[2] - lo[2]] = world[a[0]:b[0], a[1]:b[1], a[2]:b[2]]
    return out


def faces(halo, mode):
    """six bool [x, y, z] grids of the box: voxel solid, neighbour in direction d empty"""
    h = halo.copy()
    if mode == CAP:  # neighbours outside the box count as empty
        h[0], h[-1] = False, False
        h[:, 0], h[:, -1] = False, False
        h[:, :, 0], h[:, :, -1] = False, False
    X, Y, Z = (n - 2 for n in h.shape)
    solid = halo[1:-1, 1:-1, 1:-1]
    return [solid & ~h[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z] for dx, dy, dz in _STEP]


def _pack(d, s, v, u, w, h):
    a = d >> 1
    x, y, z = ((s, u, v), (u, s, v), (u, v, s))[a]
    return (np.uint32(x) | np.uint32(y) << np.uint32(10) | np.uint32(z) << np.uint32(20),
            np.uint32(w - 1) | np.uint32(h - 1) << np.uint32(10) | np.uint32(d) << np.uint32(20))


def _summary(halo, fs, quads):
    s = np.zeros(16, np.uint32)
    s[0] = halo[1:-1, 1:-1, 1:-1].sum()
    s[4:10] = [f.sum() for f in fs]
    s[1] = s[4:10].sum()
    s[2] = s[3] = len(quads)
    s[10:16] = np.bincount(quads[:, 1] >> 20, minlength=6)[:6] if len(quads) else 0
    return s


# ---- the declarative definition, vectorised ------------------------------------------------------------------------------
def _quads_of_mask(m):
    """quads (s, v, u, w, h) of the masks m[s, v, u] in ascending (s, v, u)"""
    S, V, U = m.shape
    pad = np.zeros((S, V, 1), bool)
    start = m & ~np.concatenate([pad, m[:, :, :-1]], axis=2)
    end = m & ~np.concatenate([m[:, :, 1:], pad], axis=2)  # the last bit of a run
    idx = np.broadcast_to(np.arange(U, dtype=np.int32), m.shape)
    # for every set bit the last bit of its run
    last = np.minimum.accumulate(np.where(end, idx, U)[:, :, ::-1], axis=2)[:, :, ::-1]
    run_last = np.where(start, last, -1)  # at a run's first bit: its last bit
    # the row above holds the identical run: a start at the same u with the same last bit
    above = np.concatenate([np.full((S, 1, U), -2, np.int32), run_last[:, :-1]], axis=1)
    cont = start & (above == run_last)
    qstart = start & ~cont
    # height: the rows below that continue the run at u
    height = np.zeros(m.shape, np.int32)
    below = np.zeros((S, U), np.int32)
    for v in range(V - 1, -1, -1):
        height[:, v] = 1 + below
        below = np.where(cont[:, v], height[:, v], 0)
    s, v, u = np.nonzero(qstart)
    return s, v, u, run_last[s, v, u] - u + 1, height[s, v, u]


def _triangles(d, s, v, u, w, h):
    """vertices and triangles of quads given as arrays"""
    n = len(d)
    a = d >> 1
    plane = 256 * (s + (d & 1))
    cu = 256 * np.stack([u, u + w, u + w, u], axis=1)
    cv = 256 * np.stack([v, v, v + h, v + h], axis=1)
    p = np.broadcast_to(plane[:, None], (n, 4))
    a4 = a[:, None]
    xyz = np.stack([np.where(a4 == 0, p, cu), np.where(a4 == 0, cu, np.where(a4 == 1, p, cv)), np.where(a4 == 2, p, cv)], axis=2)
    base = 4 * np.arange(n, dtype=np.int64)[:, None]
    flip = ((d & 1) == 1) == (a == 1)
    order = np.where(flip[:, None], np.array([[0, 2, 1, 0, 3, 2]]), np.array([[0, 1, 2, 0, 2, 3]]))
    return xyz.reshape(-1, 3).astype(np.int32), (base + order).reshape(-1, 3).astype(np.uint32)


def extract(world, origin, dims, mode):
    halo = halo_box(world, origin, dims)
    fs = faces(halo, mode)
    cols = [[] for _ in range(6)]
    for d in range(6):
        s, v, u, w, h = _quads_of_mask(fs[d].transpose(_SVU[d >> 1]))
        for c, x in zip(cols, (np.full(len(s), d), s, v, u, w, h)):
            c.append(np.asarray(x, np.int64))
    d, s, v, u, w, h = (np.concatenate(c) for c in cols)
    quads = np.zeros((len(d), 2), np.uint32)
    for a in range(3):
        k = (d >> 1) == a
        x, y, z = ((s, u, v), (u, s, v), (u, v, s))[a]
        quads[k, 0] = (x[k] | y[k] << 10 | z[k] << 20).astype(np.uint32)
    quads[:, 1] = ((w - 1) | (h - 1) << 10 | d << 20).astype(np.uint32)
    verts, tris = _triangles(d, s, v, u, w, h)
    return Surface(quads, verts, tris, _summary(halo, fs, quads))


# ---- a plain scan that keeps the open runs -------------------------------------------------------------------------------
def _runs(row):
    out, u, n = [], 0, len(row)
    while u < n:
        if row[u]:
            e = u
            while e < n and row[e]:
                e += 1
            out.append((u, e - u))
            u = e
        else:
            u += 1
    return out


def extract_scan(world, origin, dims, mode):
    halo = halo_box(world, origin, dims)
    fs = faces(halo, mode)
    recs = []  # [d, s, v, u, w, h]
    for d in range(6):
        m = fs[d].transpose(_SVU[d >> 1])
        for s in range(m.shape[0]):
            if not m[s].any():
                continue
            open_runs = {}
            for v in range(m.shape[1]):
                now = {}
                for run in _runs(m[s, v]):
                    if run in open_runs:
                        q = open_runs[run]
                        q[5] += 1
                    else:
                        q = [d, s, v, run[0], run[1], 1]
                        recs.append(q)
                    now[run] = q
                open_runs = now
    recs.sort(key=lambda q: q[:4])
    quads = np.zeros((len(recs), 2), np.uint32)
    verts = np.zeros((4 * len(recs), 3), np.int32)
    tris = np.zeros((2 * len(recs), 3), np.uint32)
    for i, (d, s, v, u, w, h) in enumerate(recs):
        quads[i] = _pack(d, s, v, u, w, h)
        a = d >> 1
        for c, (cu, cv) in enumerate(((u, v), (u + w, v), (u + w, v + h), (u, v + h))):
            p = [0, 0, 0]
            p[a] = s + (d & 1)
            p[(1, 0, 0)[a]] = cu
            p[(2, 2, 1)[a]] = cv
            verts[4 * i + c] = [256 * x for x in p]
        # choose the winding by the normal itself
        c0, c1, c2 = (verts[4 * i + c].astype(np.int64) for c in (0, 1, 2))
        nrm = np.cross(c1 - c0, c2 - c0)
        fwd = nrm[a] * _STEP[d][a] > 0
        tris[2 * i] = [4 * i, 4 * i + 1, 4 * i + 2] if fwd else [4 * i, 4 * i + 2, 4 * i + 1]
        tris[2 * i + 1] = [4 * i, 4 * i + 2, 4 * i + 3] if fwd else [4 * i, 4 * i + 3, 4 * i + 2]
    return Surface(quads, verts, tris, _summary(halo, fs, quads))


def decode(quads):
    """(d, x, y, z, w, h) arrays of packed quads"""
    q = np.asarray(quads, np.uint32).reshape(-1, 2)
    pos, ext = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)
    return ext >> 20, pos & 1023, pos >> 10 & 1023, pos >> 20 & 1023, (ext & 1023) + 1, (ext >> 10 & 1023) + 1


def random_world(rng, shape, density):
    return rng.random(shape) < density
