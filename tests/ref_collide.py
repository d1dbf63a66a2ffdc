"""Two restatements of the box collision queries (include/vxrt.h, vxrt_move_boxes / vxrt_overlap_boxes) on a bool [x, y, z]
grid: ``move_boxes`` / ``overlap_boxes`` vectorised over the bodies with numpy (box counts from a summed-volume table, the
nearest solid slab by a binary search on those counts), and ``move_boxes_scalar`` / ``overlap_boxes_scalar``, a per-voxel
Python loop that follows the header's wording line by line.  Every float operation is one binary32 numpy operation.

``origin`` places the grid: grid voxel (i, j, k) is world voxel origin + (i, j, k), and every world voxel outside the grid
is empty.  A grid read with vxrt_read_region at ``origin`` therefore answers exactly for bodies whose swept boxes it holds."""
from __future__ import annotations

import numpy as np

BLOCKED = (1, 2, 4)
INVALID = 8
MAX_EXTENT = np.float32(64)
MAX_DELTA = np.float32(64)
MAX_COORD = np.float32(2.0 ** 24)
F32 = np.float32


def valid(bodies) -> np.ndarray:
    """the per-body validity rule of include/vxrt.h"""
    b = np.asarray(bodies, F32).reshape(-1, 9)
    lo, hi, d = b[:, 0:3], b[:, 3:6], b[:, 6:9]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(b).all(1)
        ok &= ((lo > -MAX_COORD) & (lo < MAX_COORD) & (hi > -MAX_COORD) & (hi < MAX_COORD)).all(1)
        ok &= (lo < hi).all(1) & ((hi - lo) <= MAX_EXTENT).all(1)
        ok &= ((d >= -MAX_DELTA) & (d <= MAX_DELTA)).all(1)
    return ok


# ---- vectorised ----------------------------------------------------------------------------------------------------------
class _Counts:
    """solid voxels of inclusive world boxes, vectorised: a summed-volume table of the grid, ranges clipped to it"""

    def __init__(self, vox, origin):
        v = np.asarray(vox, bool)
        self.shape = np.asarray(v.shape, np.int64)
        self.origin = np.asarray(origin, np.int64)
        s = np.zeros(tuple(self.shape + 1), np.int64)
        s[1:, 1:, 1:] = v.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
        self.s = s

    def count(self, a0, a1):
        """a0, a1: (n, 3) int64 inclusive world voxel boxes (possibly empty) -> (n,) solid voxels"""
        lo = np.clip(a0 - self.origin, 0, self.shape)
        hi = np.clip(a1 - self.origin + 1, 0, self.shape)
        hi = np.maximum(hi, lo)
        s = self.s
        x0, y0, z0 = lo.T
        x1, y1, z1 = hi.T
        return (s[x1, y1, z1] - s[x0, y1, z1] - s[x1, y0, z1] - s[x1, y1, z0] + s[x0, y0, z1] + s[x0, y1, z0]
                + s[x1, y0, z0] - s[x0, y0, z0])


def _cover(lo, hi):
    return np.floor(lo).astype(np.int64), np.ceil(hi).astype(np.int64) - 1


def _nearest(cnt, a, s0, s1, r0, r1, forward):
    """least (forward) or greatest v in [s0, s1] whose slab of the cross-section r0 .. r1 holds a solid voxel; found mask"""
    n = len(s0)
    b0, b1 = r0.copy(), r1.copy()
    b0[:, a], b1[:, a] = s0, s1
    found = (s0 <= s1) & (cnt.count(b0, b1) > 0)
    lo, hi = s0.copy(), s1.copy()
    while True:
        act = found & (lo < hi)
        if not act.any():
            break
        mid = np.where(act, (lo + hi) // 2 if forward else (lo + hi + 1) // 2, lo)
        b0, b1 = r0.copy(), r1.copy()
        if forward:  # any solid in [s0, mid]?
            b0[:, a], b1[:, a] = s0, mid
        else:        # any solid in [mid, s1]?
            b0[:, a], b1[:, a] = mid, s1
        hit = cnt.count(b0, b1) > 0
        if forward:
            hi = np.where(act & hit, mid, hi)
            lo = np.where(act & ~hit, mid + 1, lo)
        else:
            lo = np.where(act & hit, mid, lo)
            hi = np.where(act & ~hit, mid - 1, hi)
    assert len(lo) == n
    return lo, found


def move_boxes(vox, bodies, order=(1, 0, 2), origin=(0, 0, 0)):
    """(n, 9) float32 bodies -> (lohi (n, 6) float32, flags (n,) uint32)"""
    b = np.array(bodies, F32).reshape(-1, 9)
    ok = valid(b)
    lo, hi, d = b[:, 0:3].copy(), b[:, 3:6].copy(), b[:, 6:9]
    flags = np.where(ok, 0, INVALID).astype(np.uint32)
    cnt = _Counts(vox, origin)
    for a in order:
        da = d[:, a]
        for pos in (True, False):
            m = ok & ((da > 0) if pos else (da < 0))
            if not m.any():
                continue
            l, h, dd = lo[m], hi[m], da[m]
            r0, r1 = _cover(l, h)
            if pos:
                e = h[:, a] + dd
                s0, s1 = np.ceil(h[:, a]).astype(np.int64), np.ceil(e).astype(np.int64) - 1
            else:
                e = l[:, a] + dd
                s0, s1 = np.floor(e).astype(np.int64), np.floor(l[:, a]).astype(np.int64) - 1
            v, found = _nearest(cnt, a, s0, s1, r0, r1, pos)
            nl, nh = l[:, a].copy(), h[:, a].copy()
            if pos:
                ff = v.astype(F32)
                nl = np.where(found, l[:, a] + (ff - h[:, a]), l[:, a] + dd)
                nh = np.where(found, ff, e)
            else:
                g1 = (v + 1).astype(F32)
                nh = np.where(found, h[:, a] + (g1 - l[:, a]), h[:, a] + dd)
                nl = np.where(found, g1, e)
            lo[m, a], hi[m, a] = nl, nh
            flags[np.flatnonzero(m)[found]] |= np.uint32(BLOCKED[a])
    return np.concatenate([lo, hi], 1).astype(F32), flags


def overlap_boxes(vox, bodies, origin=(0, 0, 0)):
    """(n, 9) float32 bodies -> (counts (n,) uint32, flags (n,) uint32)"""
    b = np.array(bodies, F32).reshape(-1, 9)
    ok = valid(b)
    counts = np.zeros(len(b), np.uint32)
    if ok.any():
        r0, r1 = _cover(b[ok, 0:3], b[ok, 3:6])
        counts[ok] = _Counts(vox, origin).count(r0, r1)
    return counts, np.where(ok, 0, INVALID).astype(np.uint32)


# ---- scalar, per voxel ---------------------------------------------------------------------------------------------------
def _solid(vox, origin, x, y, z):
    i, j, k = x - origin[0], y - origin[1], z - origin[2]
    return 0 <= i < vox.shape[0] and 0 <= j < vox.shape[1] and 0 <= k < vox.shape[2] and bool(vox[i, j, k])


def _slab_solid(vox, origin, a, v, lo, hi):
    rng = [range(int(np.floor(lo[k])), int(np.ceil(hi[k]))) for k in range(3)]
    rng[a] = [v]
    return any(_solid(vox, origin, x, y, z) for x in rng[0] for y in rng[1] for z in rng[2])


def move_body_scalar(vox, body, order=(1, 0, 2), origin=(0, 0, 0)):
    b = [F32(v) for v in np.asarray(body, F32).reshape(9)]
    lo, hi, delta = b[0:3], b[3:6], b[6:9]
    if not valid(np.asarray(b, F32))[0]:
        return np.asarray(lo + hi, F32), INVALID
    flags = 0
    for a in order:
        d = delta[a]
        if d == 0:
            continue
        if d > 0:
            e = F32(hi[a] + d)
            F = None
            for v in range(int(np.ceil(hi[a])), int(np.ceil(e))):
                if _slab_solid(vox, origin, a, v, lo, hi):
                    F = v
                    break
            if F is not None:
                lo[a] = F32(lo[a] + F32(F32(F) - hi[a]))
                hi[a] = F32(F)
                flags |= BLOCKED[a]
            else:
                lo[a] = F32(lo[a] + d)
                hi[a] = e
        else:
            e = F32(lo[a] + d)
            G = None
            for v in range(int(np.floor(lo[a])) - 1, int(np.floor(e)) - 1, -1):
                if _slab_solid(vox, origin, a, v, lo, hi):
                    G = v
                    break
            if G is not None:
                hi[a] = F32(hi[a] + F32(F32(G + 1) - lo[a]))
                lo[a] = F32(G + 1)
                flags |= BLOCKED[a]
            else:
                lo[a] = e
                hi[a] = F32(hi[a] + d)
    return np.asarray(lo + hi, F32), flags


def move_boxes_scalar(vox, bodies, order=(1, 0, 2), origin=(0, 0, 0)):
    out = [move_body_scalar(vox, b, order, origin) for b in np.asarray(bodies, F32).reshape(-1, 9)]
    return (np.asarray([o[0] for o in out], F32).reshape(-1, 6), np.asarray([o[1] for o in out], np.uint32))


def overlap_boxes_scalar(vox, bodies, origin=(0, 0, 0)):
    counts, flags = [], []
    for b in np.asarray(bodies, F32).reshape(-1, 9):
        if not valid(b)[0]:
            counts.append(0)
            flags.append(INVALID)
            continue
        rng = [range(int(np.floor(b[k])), int(np.ceil(b[3 + k]))) for k in range(3)]
        counts.append(sum(_solid(vox, origin, x, y, z) for x in rng[0] for y in rng[1] for z in rng[2]))
        flags.append(0)
    return np.asarray(counts, np.uint32), np.asarray(flags, np.uint32)


def swept_box(body, pad=1):
    """an integer world box (origin, dims) holding every voxel a move or overlap of ``body`` can read"""
    b = np.asarray(body, np.float64).reshape(9)
    lo = np.floor(np.minimum(b[0:3], b[0:3] + b[6:9])).astype(np.int64) - pad
    hi = np.ceil(np.maximum(b[3:6], b[3:6] + b[6:9])).astype(np.int64) + pad
    return lo, hi - lo


def random_bodies(rng, dims, n, small=False):
    """(n, 9) float32 bodies for a world of ``dims`` voxels: mostly player-sized boxes with small steps, faces often on voxel
    faces, some boxes and steps at the limits (extent 64, |delta| 64), some half or wholly outside the world, zero and -0
    steps, and a few invalid bodies.  ``small``: extents and steps of at most 6 voxels (for the per-voxel loop)."""
    dims = np.asarray(dims, np.float64)
    c = rng.uniform(-6, dims + 6, (n, 3))
    ext = rng.uniform(0.3, 3.0, (n, 3))
    d = rng.uniform(-2.0, 2.0, (n, 3))
    if small:
        ext = np.where(rng.random((n, 3)) < 0.3, rng.uniform(0.1, 6, (n, 3)), ext)
        d = np.where(rng.random((n, 3)) < 0.3, rng.uniform(-6, 6, (n, 3)), d)
    else:
        big = rng.random(n) < 0.1
        ext[big] = rng.uniform(1, 64, (int(big.sum()), 3))
        lim = rng.random((n, 3)) < 0.03
        ext[lim] = 64.0
        far = rng.random((n, 3)) < 0.1
        d[far] = rng.uniform(-64, 64, int(far.sum()))
        dl = rng.random((n, 3)) < 0.03
        d[dl] = np.where(rng.random(int(dl.sum())) < 0.5, -64.0, 64.0)
    snap = rng.random(n) < 0.4  # faces on voxel faces, integer and half-integer steps
    c[snap] = np.round(c[snap] * 2) / 2
    ext[snap] = np.maximum(np.round(ext[snap]), 1.0)
    d[snap] = np.round(d[snap] * 2) / 2
    lo = c - ext / 2
    if not small:
        edge = rng.random(n) < 0.05  # half outside the world on one axis
        ax = rng.integers(0, 3, n)
        sel = np.flatnonzero(edge)
        lo[sel, ax[sel]] = np.where(rng.random(len(sel)) < 0.5, -ext[sel, ax[sel]] / 2, dims[ax[sel]] - ext[sel, ax[sel]] / 2)
    b = np.concatenate([lo, lo + ext, d], 1).astype(F32)
    b[:, 3:6] = np.maximum(b[:, 3:6], np.nextafter(b[:, 0:3], F32(np.inf)))  # lo < hi after rounding
    b[:, 3:6] = np.minimum(b[:, 3:6], b[:, 0:3] + F32(64))
    z = rng.random((n, 3)) < 0.1
    b[:, 6:9][z] = np.where(rng.random(int(z.sum())) < 0.5, F32(0.0), F32(-0.0))
    bad = np.flatnonzero(rng.random(n) < 0.01)
    for i in bad:
        k = int(rng.integers(0, 9))
        b[i, k] = rng.choice([np.nan, np.inf, -np.inf, 1e30])
    return b
