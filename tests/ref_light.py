"""Independent restatements of the voxel light field (include/vxrt.h, vxrt_light_field) over a dense boolean world
[x, y, z] (True = solid, +y up, outside the world is empty).  Each works on the halo box [origin - 14, origin + dims + 14)
plus the full columns above it, and shares no code path with the others beyond the packing of the result:
  light_field        numpy: the level sets S_15 .. S_1 by 6-neighbour dilation masked with the empty voxels; exposure from a
                     "blocked above" mask of the columns over the halo and a downward pass through its rows.
  light_field_relax  relaxation to the fixed point L = max(L, max6(L) - 1) on the empty voxels until nothing changes
                     (scipy.ndimage.maximum_filter with the cross footprint when scipy imports, numpy shifts otherwise);
                     exposure from a cumulative OR down the whole tall column.
  light_field_brute  pure Python on the world itself, for tiny boxes: a breadth-first search through the empty voxels from
                     every voxel of B (g(s, v) is symmetric, so the search from v finds g for every source at once) and the
                     maximum of level(s) - g over the sources met.  Takes the halo as a parameter: 14 and 20 must agree.
Each returns {"levels": uint8 [x, y, z] = (sky << 4) | block, "summary": (solid, exposed, hist_sky, hist_block, sum_sky,
sum_block, used, solid_emitters, far, invalid)} with the histograms as 16-tuples.
TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/ alone."""
from __future__ import annotations

from collections import deque

import numpy as np

SKY, BLOCK = 1, 2
MAX, HALO = 15, 14
MAX_EMITTERS = 65536
SUMMARY_WORDS = 42


def have_scipy() -> bool:
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except ImportError:
        return False


def pack(sky: np.ndarray, block: np.ndarray, solid_box: np.ndarray, exposed_box, counts) -> dict:
    """the result from the two level grids of B, B's solid voxels, its exposed voxels (None without the sky channel) and the
    four emitter counts"""
    sky, block = np.asarray(sky, np.int64), np.asarray(block, np.int64)
    empty = ~np.asarray(solid_box, bool)
    hist = lambda a: tuple(int(v) for v in np.bincount(a[empty].ravel(), minlength=16))
    return {"levels": (sky << 4 | block).astype(np.uint8),
            "summary": (int((~empty).sum()), 0 if exposed_box is None else int(np.asarray(exposed_box).sum()), hist(sky), hist(block),
                        int(sky.sum()), int(block.sum()), *(int(c) for c in counts))}


def summary_from_words(w) -> tuple:
    """vxrt_light_summary (42 uint32 words) in the form of the restatements' summaries"""
    w = [int(v) for v in np.asarray(w).view(np.uint32)]
    return (w[0], w[1], tuple(w[2:18]), tuple(w[18:34]), w[34] | w[35] << 32, w[36] | w[37] << 32, w[38], w[39], w[40], w[41])


def _emitters(emitters) -> np.ndarray:
    return np.zeros((0, 4), np.int64) if emitters is None else np.asarray(emitters, np.int64).reshape(-1, 4)


# ---- (a) level sets -------------------------------------------------------------------------------------------------------
def halo_solid(world: np.ndarray, origin, dims, halo: int = HALO) -> np.ndarray:
    """the solid voxels of the halo box; halo voxel 0 is world voxel origin - halo"""
    world = np.asarray(world, bool)
    shape = tuple(int(d) + 2 * halo for d in dims)
    solid = np.zeros(shape, bool)
    src, dst = [], []
    for k in range(3):
        lo = int(origin[k]) - halo
        a, b = max(lo, 0), min(lo + shape[k], world.shape[k])
        if a >= b:
            return solid
        src.append(slice(a, b))
        dst.append(slice(a - lo, b - lo))
    solid[tuple(dst)] = world[tuple(src)]
    return solid


def blocked_above(world: np.ndarray, origin, dims, halo: int = HALO) -> np.ndarray:
    """per (x, z) of the halo box: some solid voxel of the world above the halo's top row"""
    world = np.asarray(world, bool)
    hx, hz = int(dims[0]) + 2 * halo, int(dims[2]) + 2 * halo
    out = np.zeros((hx, hz), bool)
    top = max(int(origin[1]) + int(dims[1]) + halo, 0)
    if top >= world.shape[1]:
        return out
    lox, loz = int(origin[0]) - halo, int(origin[2]) - halo
    ax, bx = max(lox, 0), min(lox + hx, world.shape[0])
    az, bz = max(loz, 0), min(loz + hz, world.shape[2])
    if ax < bx and az < bz:
        out[ax - lox:bx - lox, az - loz:bz - loz] = world[ax:bx, top:, az:bz].any(axis=1)
    return out


def _dilate6(s: np.ndarray) -> np.ndarray:
    out = s.copy()
    out[1:] |= s[:-1]
    out[:-1] |= s[1:]
    out[:, 1:] |= s[:, :-1]
    out[:, :-1] |= s[:, 1:]
    out[:, :, 1:] |= s[:, :, :-1]
    out[:, :, :-1] |= s[:, :, 1:]
    return out


def _level_sets(empty: np.ndarray, source: np.ndarray) -> np.ndarray:
    """level = how many of S_15 .. S_1 hold the voxel; source: the source level per voxel (0: none), on empty voxels only"""
    level = np.zeros(empty.shape, np.int64)
    s = np.zeros(empty.shape, bool)
    for k in range(MAX, 0, -1):
        s = (_dilate6(s) | (source == k)) & empty
        level += s
    return level


def light_field(world, origin, dims, emitters=None, channels: int = SKY | BLOCK) -> dict:
    H = HALO
    solid = halo_solid(world, origin, dims)
    empty = ~solid
    box = tuple(slice(H, H + int(d)) for d in dims)
    sky = block = np.zeros(tuple(int(d) for d in dims), np.int64)
    exposed_box, counts = None, (0, 0, 0, 0)
    if channels & SKY:
        exposed = np.zeros(solid.shape, bool)
        run = ~blocked_above(world, origin, dims)
        for y in range(solid.shape[1] - 1, -1, -1):
            run = run & empty[:, y, :]
            exposed[:, y, :] = run
        sky = _level_sets(empty, np.where(exposed, MAX, 0))[box]
        exposed_box = exposed[box]
    if channels & BLOCK:
        e = _emitters(emitters)
        valid = (e[:, 3] >= 1) & (e[:, 3] <= MAX)
        h = e[:, :3] - (np.asarray(origin, np.int64) - H)
        near = valid & ((h >= 0) & (h < np.asarray(solid.shape, np.int64))).all(axis=1)
        hn = h[near]
        on_solid = solid[hn[:, 0], hn[:, 1], hn[:, 2]]
        source = np.zeros(solid.shape, np.int64)
        used = hn[~on_solid]
        np.maximum.at(source, (used[:, 0], used[:, 1], used[:, 2]), e[near][~on_solid][:, 3])
        block = _level_sets(empty, source)[box]
        counts = (len(used), int(on_solid.sum()), int((valid & ~near).sum()), int((~valid).sum()))
    return pack(sky, block, solid[box], exposed_box, counts)


# ---- (b) relaxation ---------------------------------------------------------------------------------------------------------
def _relax(empty: np.ndarray, source: np.ndarray) -> np.ndarray:
    L = np.where(empty, source, 0).astype(np.int64)
    if have_scipy():
        from scipy import ndimage
        cross = ndimage.generate_binary_structure(3, 1)
        spread = lambda a: ndimage.maximum_filter(a, footprint=cross, mode="constant", cval=0)
    else:
        def spread(a):
            p = np.pad(a, 1)
            return np.maximum.reduce([p[1:-1, 1:-1, 1:-1], p[2:, 1:-1, 1:-1], p[:-2, 1:-1, 1:-1], p[1:-1, 2:, 1:-1],
                                      p[1:-1, :-2, 1:-1], p[1:-1, 1:-1, 2:], p[1:-1, 1:-1, :-2]])
    while True:
        nxt = np.where(empty, np.maximum(L, spread(L) - 1), 0)
        if np.array_equal(nxt, L):
            return L
        L = nxt


def light_field_relax(world, origin, dims, emitters=None, channels: int = SKY | BLOCK) -> dict:
    world = np.asarray(world, bool)
    H = HALO
    o = [int(v) for v in origin]
    d = [int(v) for v in dims]
    # the tall box: the halo in x and z, from the halo's bottom row to the world's top (or the halo's, if that is higher)
    ylo, yhi = o[1] - H, max(o[1] + d[1] + H, world.shape[1])
    tall = np.zeros((d[0] + 2 * H, yhi - ylo, d[2] + 2 * H), bool)
    for ix in range(tall.shape[0]):
        x = o[0] - H + ix
        if 0 <= x < world.shape[0]:
            for iz in range(tall.shape[2]):
                z = o[2] - H + iz
                if 0 <= z < world.shape[2]:
                    a, b = max(ylo, 0), min(yhi, world.shape[1])
                    if a < b:
                        tall[ix, a - ylo:b - ylo, iz] = world[x, a:b, z]
    hy = d[1] + 2 * H
    solid = tall[:, :hy, :]
    empty = ~solid
    box = (slice(H, H + d[0]), slice(H, H + d[1]), slice(H, H + d[2]))
    sky = block = np.zeros(tuple(d), np.int64)
    exposed_box, counts = None, [0, 0, 0, 0]
    if channels & SKY:
        covered = np.logical_or.accumulate(tall[:, ::-1, :], axis=1)[:, ::-1, :]  # solid at this row or above
        exposed = ~covered[:, :hy, :]
        sky = _relax(empty, np.where(exposed, MAX, 0))[box]
        exposed_box = exposed[box]
    if channels & BLOCK:
        source = np.zeros(solid.shape, np.int64)
        for x, y, z, level in _emitters(emitters).tolist():
            p = (x - o[0] + H, y - o[1] + H, z - o[2] + H)
            if not 1 <= level <= MAX:
                counts[3] += 1
            elif not all(0 <= p[k] < solid.shape[k] for k in range(3)):
                counts[2] += 1
            elif solid[p]:
                counts[1] += 1
            else:
                counts[0] += 1
                source[p] = max(source[p], level)
        block = _relax(empty, source)[box]
    return pack(sky, block, solid[box], exposed_box, counts)


# ---- (c) brute force ----------------------------------------------------------------------------------------------------------
def light_field_brute(world, origin, dims, emitters=None, channels: int = SKY | BLOCK, halo: int = HALO) -> dict:
    world = np.asarray(world, bool)
    X, Y, Z = world.shape
    o = [int(v) for v in origin]
    d = [int(v) for v in dims]
    lo = [o[k] - halo for k in range(3)]
    hi = [o[k] + d[k] + halo for k in range(3)]  # exclusive
    inside = lambda p: all(lo[k] <= p[k] < hi[k] for k in range(3))
    is_solid = lambda p: 0 <= p[0] < X and 0 <= p[1] < Y and 0 <= p[2] < Z and bool(world[p])
    seen_exposed = {}

    def exposed(p):
        if p not in seen_exposed:
            x, y, z = p
            seen_exposed[p] = not is_solid(p) and not (0 <= x < X and 0 <= z < Z and y < Y and bool(world[x, max(y, 0):, z].any()))
        return seen_exposed[p]

    lamp, counts = {}, [0, 0, 0, 0]
    if channels & BLOCK:
        for x, y, z, level in _emitters(emitters).tolist():
            p = (x, y, z)
            cls = 3 if level < 1 or level > MAX else 2 if not inside(p) else 1 if is_solid(p) else 0
            counts[cls] += 1
            if cls == 0:
                lamp[p] = max(lamp.get(p, 0), level)
    sky, block = np.zeros(tuple(d), np.int64), np.zeros(tuple(d), np.int64)
    solid_box, exposed_box = np.zeros(tuple(d), bool), np.zeros(tuple(d), bool)
    for ix in range(d[0]):
        for iy in range(d[1]):
            for iz in range(d[2]):
                v = (o[0] + ix, o[1] + iy, o[2] + iz)
                if is_solid(v):
                    solid_box[ix, iy, iz] = True
                    continue
                exposed_box[ix, iy, iz] = bool(channels & SKY) and exposed(v)
                best_sky = best_block = 0
                dist = {v: 0}
                queue = deque([v])
                while queue:
                    p = queue.popleft()
                    g = dist[p]
                    if channels & SKY and exposed(p):
                        best_sky = max(best_sky, MAX - g)
                    if p in lamp:
                        best_block = max(best_block, lamp[p] - g)
                    if g == MAX - 1:
                        continue
                    for k in range(3):
                        for s in (-1, 1):
                            q = tuple(p[j] + (s if j == k else 0) for j in range(3))
                            if q not in dist and inside(q) and not is_solid(q):
                                dist[q] = g + 1
                                queue.append(q)
                sky[ix, iy, iz], block[ix, iy, iz] = best_sky, best_block
    return pack(sky, block, solid_box, exposed_box if channels & SKY else None, counts)


def leaky_roof_world(rng, shape=(64, 48, 64), density=0.45, roof_y=30, roof_density=0.9) -> np.ndarray:
    """noise with a y-layer that is mostly solid: light leaks through the roof's holes and fades in the caves below it, so a
    box that straddles the roof shows every level (uniform noise gives only dark or only bright fields)"""
    w = rng.random(shape) < density
    w[:, roof_y, :] = rng.random((shape[0], shape[2])) < roof_density
    return w
