"""Independent restatements of the loose voxels (include/vxrt.h, vxrt_loose_step) over a dense boolean world [x, y, z] (True =
solid) and a loose layer, a bool [x, y, z] grid of the box's dims.
  loose_step_sets   pure Python over sets of world coordinates: every pass scans the layer voxel by voxel and decides each
                    move from a snapshot of the layer before the pass; blocked and sink are functions of a coordinate.
  loose_step        numpy: the layer, the blocked and the live voxels as arrays over the halo box (the box grown by one
                    voxel), every pass as shifted copies of them; the direction of a voxel from arrays of world coordinates.
Each returns {"bits": bool [x, y, z] of the box, "summary": (loose_in, loose_start, loose_after, fell_last, slid_last,
spread_last, changed_min, changed_max)} with the two corners as 3-tuples; with keep_passes also "passes": per pass
(step t, pass, movers as (source, target) world coordinates -- the set version only) and "drained".
TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/ alone."""
from __future__ import annotations

import numpy as np

SAND, WATER = 0, 1
WALL, OPEN = 0, 1
FALL, SLIDE, SPREAD = 0, 1, 2
MAX_STEPS = 64
SUMMARY_WORDS = 12
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
NONE = ((INT_MAX,) * 3, (INT_MIN,) * 3)


def passes_of(material: int) -> tuple:
    return (FALL, SLIDE, SPREAD) if material == WATER else (FALL, SLIDE)


def direction(v, t: int) -> tuple:
    """d(v) of step t: the axis t & 1 (0: x, 1: z), the sign from the parity of c + y + (t >> 1)"""
    a = t & 1
    c = v[2] if a == 0 else v[0]
    sign = 1 if (c + v[1] + (t >> 1)) & 1 == 0 else -1
    return (sign, 0, 0) if a == 0 else (0, 0, sign)


def summary_from_words(w) -> tuple:
    """vxrt_loose_summary (12 words) in the form of the restatements' summaries"""
    w = np.ascontiguousarray(np.asarray(w).view(np.uint32)[:12])
    box = [int(v) for v in w[6:12].view(np.int32)]
    return (*(int(v) for v in w[:6]), tuple(box[:3]), tuple(box[3:]))


def _changed_box(origin, before, after):
    ch = np.argwhere(before != after)
    if not len(ch):
        return NONE
    return (tuple(int(v) + int(o) for v, o in zip(ch.min(axis=0), origin)), tuple(int(v) + int(o) for v, o in zip(ch.max(axis=0), origin)))


# ---- (a) sets -----------------------------------------------------------------------------------------------------------------
def loose_step_sets(world, origin, dims, loose, material=SAND, steps=1, edge=WALL, phase=0, keep_passes=False) -> dict:
    world = np.asarray(world, bool)
    loose = np.asarray(loose, bool)
    S = world.shape
    o = [int(v) for v in origin]
    d = [int(v) for v in dims]
    assert loose.shape == tuple(d)
    in_world = lambda p: 0 <= p[0] < S[0] and 0 <= p[1] < S[1] and 0 <= p[2] < S[2]
    in_box = lambda p: all(o[k] <= p[k] < o[k] + d[k] for k in range(3))
    live = lambda p: in_box(p) and in_world(p)
    solid = lambda p: in_world(p) and bool(world[p])

    def blocked(p):
        return solid(p) if live(p) or edge == OPEN else True

    layer = set()
    for i in np.argwhere(loose):
        p = (o[0] + int(i[0]), o[1] + int(i[1]), o[2] + int(i[2]))
        if live(p) and not solid(p):
            layer.add(p)
    start = len(layer)
    counts, passes, drained = [0, 0, 0], [], 0
    for i in range(steps):
        t = (phase + i) & 0xFFFFFFFF
        counts = [0, 0, 0]
        for kind in passes_of(material):
            snap = frozenset(layer)
            free = lambda p: not blocked(p) and p not in snap
            moves = []
            for v in snap:
                below = (v[0], v[1] - 1, v[2])
                if kind == FALL:
                    if free(below):
                        moves.append((v, below))
                    continue
                if free(below):
                    continue  # not resting
                dx, _, dz = direction(v, t)
                side = (v[0] + dx, v[1], v[2] + dz)
                if kind == SLIDE:
                    target = (side[0], side[1] - 1, side[2])
                    if free(side) and free(target):
                        moves.append((v, target))
                elif free(side):
                    moves.append((v, side))
            targets = [m[1] for m in moves]
            assert len(set(targets)) == len(targets), "two movers share a target"
            for v, target in moves:
                layer.remove(v)
            for v, target in moves:
                if live(target):
                    assert target not in layer
                    layer.add(target)
                else:  # a sink
                    assert edge == OPEN and not blocked(target)
                    drained += 1
            counts[kind] = len(moves)
            passes.append((t, kind, moves))
    out = np.zeros(tuple(d), bool)
    for p in layer:
        out[p[0] - o[0], p[1] - o[1], p[2] - o[2]] = True
    r = {"bits": out, "summary": (int(loose.sum()), start, len(layer), *counts, *_changed_box(o, loose, out))}
    if keep_passes:
        r["passes"], r["drained"] = passes, drained
    return r


# ---- (b) numpy over the halo box ------------------------------------------------------------------------------------------
def _halo(world, origin, dims):
    """(solid, in-world) over the halo box [origin - 1, origin + dims + 1)"""
    shape = tuple(int(v) + 2 for v in dims)
    w, inw = np.zeros(shape, bool), np.zeros(shape, bool)
    src, dst = [], []
    for k in range(3):
        lo = int(origin[k]) - 1
        a, b = max(lo, 0), min(lo + shape[k], world.shape[k])
        if a >= b:
            return w, inw
        src.append(slice(a, b))
        dst.append(slice(a - lo, b - lo))
    w[tuple(dst)] = world[tuple(src)]
    inw[tuple(dst)] = True
    return w, inw


def _at(a: np.ndarray, off) -> np.ndarray:
    """a[v + off] for every v; False where v + off leaves the array"""
    out = np.zeros_like(a)
    s_dst, s_src = [], []
    for n, k in zip(a.shape, off):
        s_dst.append(slice(max(-k, 0), n - max(k, 0)))
        s_src.append(slice(max(k, 0), n - max(-k, 0)))
    out[tuple(s_dst)] = a[tuple(s_src)]
    return out


def loose_step(world, origin, dims, loose, material=SAND, steps=1, edge=WALL, phase=0) -> dict:
    world = np.asarray(world, bool)
    loose = np.asarray(loose, bool)
    d = tuple(int(v) for v in dims)
    assert loose.shape == d
    w, inw = _halo(world, origin, d)
    box = tuple(slice(1, 1 + n) for n in d)
    live = np.zeros(w.shape, bool)
    live[box] = inw[box]
    blocked = np.where(live, w, True if edge == WALL else w)
    layer = np.zeros(w.shape, bool)
    layer[box] = loose
    layer &= live & ~blocked
    start = int(layer.sum())
    gx, gy, gz = np.meshgrid(*(np.arange(n, dtype=np.int64) + int(o) - 1 for n, o in zip(w.shape, origin)), indexing="ij")
    counts = [0, 0, 0]
    for i in range(steps):
        t = (phase + i) & 0xFFFFFFFF
        counts = [0, 0, 0]
        plus = ((gz if t & 1 == 0 else gx) + gy + (t >> 1)) % 2 == 0
        axis = 0 if t & 1 == 0 else 2
        for kind in passes_of(material):
            free = ~blocked & ~layer
            below = _at(free, (0, -1, 0))
            if kind == FALL:
                movers = {(0, -1, 0): layer & below}
            else:
                movers = {}
                for sign, sel in ((1, plus), (-1, ~plus)):
                    off = [0, 0, 0]
                    off[axis] = sign
                    ok = layer & ~below & sel & _at(free, off)
                    if kind == SLIDE:
                        off[1] = -1
                        ok &= _at(free, off)
                    movers[tuple(off)] = ok
            nxt = layer.copy()
            for m in movers.values():
                nxt &= ~m
            for off, m in movers.items():
                arrive = _at(m, tuple(-k for k in off))
                assert not (nxt & arrive).any()
                nxt |= arrive & live
                counts[kind] += int(m.sum())
            layer = nxt
    out = layer[box]
    return {"bits": out, "summary": (int(loose.sum()), start, int(out.sum()), *counts, *_changed_box(origin, loose, out))}


# ---- worlds -------------------------------------------------------------------------------------------------------------------
def terrain(rng, shape=(32, 32, 32), low=1, high=4, holes=0.0) -> np.ndarray:
    """columns of random height low .. high; with `holes`, that share of the columns is empty down through the floor (leaky)"""
    X, Y, Z = shape
    h = rng.integers(low, high + 1, size=(X, Z))
    if holes:
        h[rng.random((X, Z)) < holes] = 0
    return np.arange(Y)[None, :, None] < h[:, None, :]


def random_layer(rng, dims, density=0.1) -> np.ndarray:
    return rng.random(tuple(dims)) < density


def at_rest(world, origin, dims, bits, edge=WALL) -> bool:
    """no loose voxel has a free voxel below it or an open slide, whatever the step's number"""
    for t in range(4):
        r = loose_step(world, origin, dims, bits, SAND, 1, edge, t)
        if r["summary"][3] or r["summary"][4]:
            return False
    return True
