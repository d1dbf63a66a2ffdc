"""Independent restatements of the exact distance field (include/vxrt.h, vxrt_distance_field) over a dense boolean world
[x, y, z], each building the halo [origin - R, origin + dims + R) with "outside the world is empty":
  distance_field        numpy: three separable min-plus passes in int64, each over the offsets -R .. R.
  distance_field_scipy  scipy.ndimage.distance_transform_edt(..., return_indices=True) on the halo (used when scipy imports);
                        d2 is recomputed in int64 from the returned indices, never taken from the float distances.
  distance_field_brute  O(voxels x targets), for tiny grids.
  distance_field_points the definition on a world given as a short list of voxels (no halo is built), for large radii.
Each returns {"dist2": uint16 [x, y, z] (FAR above R^2), "summary": (zero, near, far, max_d2, sum_d2)}.
TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/ alone."""
from __future__ import annotations

import numpy as np

TO_SOLID, TO_EMPTY = 0, 1
FAR = 0xFFFF
MAX_RADIUS = 255
_INF = np.int64(1) << 40


def halo_targets(world: np.ndarray, origin, dims, radius: int, mode: int) -> np.ndarray:
    """the targets of the halo box as a bool grid of dims + 2 R per axis; halo voxel 0 is world voxel origin - R"""
    world = np.asarray(world, bool)
    R = int(radius)
    shape = tuple(int(d) + 2 * R for d in dims)
    solid = np.zeros(shape, bool)
    src, dst = [], []
    for k in range(3):
        lo = int(origin[k]) - R
        a, b = max(lo, 0), min(lo + shape[k], world.shape[k])
        if a >= b:
            break
        src.append(slice(a, b))
        dst.append(slice(a - lo, b - lo))
    else:
        solid[tuple(dst)] = world[tuple(src)]
    return solid if mode == TO_SOLID else ~solid


def summarise(d2: np.ndarray) -> tuple:
    near = d2[d2 != FAR].astype(np.int64)
    return (int((near == 0).sum()), int((near > 0).sum()), int((d2 == FAR).sum()), int(near.max()) if near.size else 0,
            int(near.sum()))


def _result(d2: np.ndarray, radius: int) -> dict:
    out = np.where(d2 <= radius * radius, d2, FAR).astype(np.uint16)
    return {"dist2": out, "summary": summarise(out)}


def _pass(g: np.ndarray, axis: int, n: int, R: int) -> np.ndarray:
    """out[i] = min over |k| <= R of g[i + R + k] + k^2 along `axis`, for i < n; a bool g is 0 where set, else infinite"""
    out = None
    for k in range(-R, R + 1):
        idx = [slice(None)] * 3
        idx[axis] = slice(R + k, R + k + n)
        part = g[tuple(idx)]
        term = np.where(part, np.int64(k * k), _INF) if g.dtype == bool else part + np.int64(k * k)
        out = term if out is None else np.minimum(out, term, out=out)
    return out


def distance_field(world, origin, dims, radius: int, mode: int = TO_SOLID) -> dict:
    R = int(radius)
    g = halo_targets(world, origin, dims, R, mode)
    for axis in range(3):
        g = _pass(g, axis, int(dims[axis]), R)
    return _result(g, R)


def distance_field_scipy(world, origin, dims, radius: int, mode: int = TO_SOLID) -> dict:
    from scipy import ndimage
    R = int(radius)
    t = halo_targets(world, origin, dims, R, mode)
    box = tuple(slice(R, R + int(d)) for d in dims)
    if not t.any():
        return _result(np.full(tuple(int(d) for d in dims), _INF), R)
    idx = ndimage.distance_transform_edt(~t, return_distances=False, return_indices=True)
    d2 = np.zeros(tuple(int(d) for d in dims), np.int64)
    for k in range(3):
        shape = [1, 1, 1]
        shape[k] = int(dims[k])
        own = (np.arange(int(dims[k]), dtype=np.int64) + R).reshape(shape)
        diff = idx[k][box].astype(np.int64) - own
        d2 += diff * diff
    return _result(d2, R)


def distance_field_brute(world, origin, dims, radius: int, mode: int = TO_SOLID) -> dict:
    R = int(radius)
    t = np.argwhere(halo_targets(world, origin, dims, R, mode)).astype(np.int64) - R
    dims = tuple(int(d) for d in dims)
    v = np.stack(np.meshgrid(*[np.arange(d, dtype=np.int64) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    d2 = np.full(len(v), _INF)
    for a in range(0, len(t), 512):
        diff = v[:, None, :] - t[None, a:a + 512, :]
        d2 = np.minimum(d2, (diff * diff).sum(-1).min(1))
    return _result(d2.reshape(dims), R)


def distance_field_points(world_shape, targets, origin, dims, radius: int, mode: int = TO_SOLID) -> dict:
    """The definition itself on a world given by a short list of voxels, for radii at which the halo forms are slow.
    TO_SOLID: `targets` are the solid voxels of an otherwise empty world of `world_shape`; d2 = min over them of |p - s|^2.
    TO_EMPTY: they are the empty voxels of an otherwise solid world, and every voxel outside the world is empty too: the
    nearest of those is straight across the nearest face, so its distance is the least over the six faces.  A target with
    d2 <= R^2 is within R on every axis, so no halo is built.  O(voxels x targets)."""
    R = int(radius)
    shape = np.asarray(world_shape, np.int64)
    dims = tuple(int(d) for d in dims)
    ax = [np.arange(d, dtype=np.int64) + int(o) for o, d in zip(origin, dims)]  # world coordinates of the box
    t = np.asarray(targets, np.int64).reshape(-1, 3)
    d2 = np.full(dims, _INF)
    for s in t[((t >= 0) & (t < shape)).all(1)]:  # a listed voxel outside the world changes nothing in either mode
        sq = [(a - c) ** 2 for a, c in zip(ax, s)]
        np.minimum(d2, sq[0][:, None, None] + sq[1][None, :, None] + sq[2][None, None, :], out=d2)
    if mode == TO_EMPTY:
        steps = [np.where((a < 0) | (a >= n), 0, np.minimum(a + 1, n - a)) for a, n in zip(ax, shape)]  # 0: outside already
        out = np.minimum(np.minimum(steps[0][:, None, None], steps[1][None, :, None]), steps[2][None, None, :])
        np.minimum(d2, out * out, out=d2)
    return _result(d2, R)


def have_scipy() -> bool:
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except ImportError:
        return False


def fast(world, origin, dims, radius: int, mode: int = TO_SOLID) -> dict:
    """scipy when it imports, else numpy: for the large grids of the GPU tests"""
    return (distance_field_scipy if have_scipy() else distance_field)(world, origin, dims, radius, mode)


def ball_points(R: int) -> int:
    """lattice points p with |p|^2 <= R^2"""
    a = np.arange(-R, R + 1, dtype=np.int64)
    return int(((a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2) <= R * R).sum())
