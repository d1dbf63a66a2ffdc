"""Independent restatements of the neighbour-count voxel rules (include/vxrt.h, vxrt_apply_rule) over a dense boolean world
[x, y, z] (True = solid; a voxel outside the world has the rule's constant value `outside`).  A rule is a RefRule
(neighbours 0 / 1 / 2 for N6 / N18 / N26, born and survive as int masks, iterations, scope 0 box / 1 world, outside 0 / 1).
  apply_rule         numpy: the halo box padded by one voxel and the neighbourhood's shifted copies summed.
  apply_rule_conv    the same steps with the count from scipy.ndimage.convolve and one kernel per neighbourhood.
  apply_rule_brute   pure Python, one voxel at a time, for small boxes: a dictionary of the voxels that differ from W_0.  The
                     WORLD scope runs the rule on the whole world and a margin of iterations + 1 voxels around the world and
                     the box, never on a halo, and reads the box out at the end.
Each returns {"bits": bool [x, y, z] of the box (False outside the world), "summary": (solid_before, solid_after, born,
died, changed_last, changed_min, changed_max)} with the two corners as 3-tuples.
TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/ alone."""
from __future__ import annotations

from itertools import product
from typing import NamedTuple

import numpy as np

N6, N18, N26 = 0, 1, 2
BOX, WORLD = 0, 1
COUNT = {N6: 6, N18: 18, N26: 26}
MAX_ITERATIONS = 16
SUMMARY_WORDS = 12
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


class RefRule(NamedTuple):
    neighbours: int
    born: int
    survive: int
    iterations: int = 1
    scope: int = BOX
    outside: int = 0


def bits_of(counts) -> int:
    m = 0
    for c in counts:
        m |= 1 << c
    return m


def smooth(iterations=1, **kw) -> RefRule:
    return RefRule(N26, bits_of(range(14, 27)), bits_of(range(13, 27)), iterations, **kw)


def grow(neighbours=N26, iterations=1, **kw) -> RefRule:
    n = COUNT[neighbours]
    return RefRule(neighbours, bits_of(range(1, n + 1)), bits_of(range(0, n + 1)), iterations, **kw)


def erode(neighbours=N26, iterations=1, **kw) -> RefRule:
    return RefRule(neighbours, 0, 1 << COUNT[neighbours], iterations, **kw)


def offsets(neighbours: int) -> list:
    """the neighbourhood's offsets, by the definition: d != 0 in {-1, 0, 1}^3 with |d|_1 <= 1, 2, 3"""
    reach = {N6: 1, N18: 2, N26: 3}[neighbours]
    return [d for d in product((-1, 0, 1), repeat=3) if 1 <= abs(d[0]) + abs(d[1]) + abs(d[2]) <= reach]


def halo_of(rule: RefRule) -> int:
    return rule.iterations if rule.scope == WORLD else 1


def summary_from_words(w) -> tuple:
    """vxrt_rule_summary (12 words) in the form of the restatements' summaries"""
    w = np.ascontiguousarray(np.asarray(w).view(np.uint32)[:12])
    box = [int(v) for v in w[6:12].view(np.int32)]
    assert int(w[5]) == 0
    return (*(int(v) for v in w[:5]), tuple(box[:3]), tuple(box[3:]))


def summarize(origin, inw, w0, wn, prev) -> tuple:
    """the summary over the world voxels `inw` of the box from W_0, W_n and W_n-1 there"""
    w0, wn, prev = w0 & inw, wn & inw, prev & inw
    ch = np.argwhere(w0 != wn)
    lo = tuple(int(v) + int(o) for v, o in zip(ch.min(axis=0), origin)) if len(ch) else (INT_MAX,) * 3
    hi = tuple(int(v) + int(o) for v, o in zip(ch.max(axis=0), origin)) if len(ch) else (INT_MIN,) * 3
    return (int(w0.sum()), int(wn.sum()), int((wn & ~w0).sum()), int((w0 & ~wn).sum()), int((wn != prev).sum()), lo, hi)


# ---- (a) shifted sums, (b) convolution ----------------------------------------------------------------------------------------
def halo_world(world: np.ndarray, origin, dims, h: int, outside: int):
    """(W_0, in-world) over the halo box [origin - h, origin + dims + h)"""
    world = np.asarray(world, bool)
    shape = tuple(int(d) + 2 * h for d in dims)
    w0 = np.full(shape, bool(outside))
    inw = np.zeros(shape, bool)
    src, dst = [], []
    for k in range(3):
        lo = int(origin[k]) - h
        a, b = max(lo, 0), min(lo + shape[k], world.shape[k])
        if a >= b:
            return w0, inw
        src.append(slice(a, b))
        dst.append(slice(a - lo, b - lo))
    w0[tuple(dst)] = world[tuple(src)]
    inw[tuple(dst)] = True
    return w0, inw


def count_shifted(w: np.ndarray, neighbours: int) -> np.ndarray:
    p = np.pad(w.astype(np.int64), 1)
    X, Y, Z = w.shape
    c = np.zeros(w.shape, np.int64)
    for dx, dy, dz in offsets(neighbours):
        c += p[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
    return c


def _kernel(neighbours: int) -> np.ndarray:
    k = np.zeros((3, 3, 3), np.int64)
    i = np.arange(3) - 1
    dist = np.abs(i)[:, None, None] + np.abs(i)[None, :, None] + np.abs(i)[None, None, :]
    k[(dist >= 1) & (dist <= {N6: 1, N18: 2, N26: 3}[neighbours])] = 1
    return k


def count_convolved(w: np.ndarray, neighbours: int) -> np.ndarray:
    from scipy import ndimage
    return ndimage.convolve(w.astype(np.int64), _kernel(neighbours), mode="constant", cval=0)


def _apply(world, origin, dims, rule: RefRule, mask, counter, keep_steps=False) -> dict:
    h = halo_of(rule)
    w0, inw = halo_world(world, origin, dims, h, rule.outside)
    box = tuple(slice(h, h + int(d)) for d in dims)
    if rule.scope == WORLD:
        assert mask is None
        free = inw.copy()
    else:
        free = np.zeros(w0.shape, bool)
        free[box] = inw[box] if mask is None else inw[box] & np.asarray(mask, bool)
    w, prev, steps = w0, w0, []
    for _ in range(rule.iterations):
        c = count_shifted(w, rule.neighbours) if counter is None else counter(w, rule.neighbours)
        nxt = np.where(w, (rule.survive >> c) & 1, (rule.born >> c) & 1).astype(bool)
        prev, w = w, np.where(free, nxt, w)
        steps.append((w[box], c[box]))
    out = {"bits": w[box] & inw[box], "summary": summarize(origin, inw[box], w0[box], w[box], prev[box])}
    if keep_steps:
        out["steps"], out["free"], out["w0"] = steps, free[box], w0[box]
    return out


def apply_rule(world, origin, dims, rule: RefRule, mask=None, keep_steps=False) -> dict:
    return _apply(world, origin, dims, rule, mask, None, keep_steps)


def apply_rule_conv(world, origin, dims, rule: RefRule, mask=None) -> dict:
    return _apply(world, origin, dims, rule, mask, count_convolved)


# ---- (c) brute force --------------------------------------------------------------------------------------------------------
def apply_rule_brute(world, origin, dims, rule: RefRule, mask=None) -> dict:
    world = np.asarray(world, bool)
    S = world.shape
    o = [int(v) for v in origin]
    d = [int(v) for v in dims]
    offs = offsets(rule.neighbours)
    in_world = lambda p: 0 <= p[0] < S[0] and 0 <= p[1] < S[1] and 0 <= p[2] < S[2]
    in_box = lambda p: all(o[k] <= p[k] < o[k] + d[k] for k in range(3))

    def w0(p):
        return bool(world[p]) if in_world(p) else bool(rule.outside)

    if rule.scope == WORLD:
        assert mask is None
        m = rule.iterations + 1
        lo = [min(0, o[k]) - m for k in range(3)]
        hi = [max(S[k], o[k] + d[k]) + m for k in range(3)]
        domain = [p for p in product(*(range(lo[k], hi[k]) for k in range(3))) if in_world(p)]
    else:
        mk = None if mask is None else np.asarray(mask, bool)
        domain = [p for p in product(*(range(o[k], o[k] + d[k]) for k in range(3)))
                  if in_world(p) and (mk is None or mk[p[0] - o[0], p[1] - o[1], p[2] - o[2]])]
    cur, prev = {}, {}  # the voxels whose value differs from W_0: p -> value
    value = lambda state, p: state[p] if p in state else w0(p)
    for _ in range(rule.iterations):
        nxt = {}
        for p in domain:
            c = sum(value(cur, (p[0] + a, p[1] + b, p[2] + e)) for a, b, e in offs)
            v = bool(((rule.survive if value(cur, p) else rule.born) >> c) & 1)
            if v != w0(p):
                nxt[p] = v
        prev, cur = cur, nxt
    shape = tuple(d)
    inw, a0, an, ap = (np.zeros(shape, bool) for _ in range(4))
    for i in product(*(range(n) for n in d)):
        p = (o[0] + i[0], o[1] + i[1], o[2] + i[2])
        inw[i], a0[i], an[i], ap[i] = in_world(p), w0(p), value(cur, p), value(prev, p)
    assert all(in_box(p) for p in cur) or rule.scope == WORLD
    return {"bits": an & inw, "summary": summarize(o, inw, a0, an, ap)}


# ---- worlds --------------------------------------------------------------------------------------------------------------------
def gradient_world(rng, shape=(64, 64, 64)) -> np.ndarray:
    """solid density rising from 0 to 1 along x: every neighbour count 0 .. 26 occurs around solid and around empty voxels"""
    ramp = (np.arange(shape[0]) + 0.5) / shape[0]
    return rng.random(shape) < ramp[:, None, None]


def random_rule(rng, neighbours, iterations=1, scope=BOX, outside=0) -> RefRule:
    """random tables over 0 .. N, neither empty nor full"""
    n = COUNT[neighbours]
    full = (2 << n) - 1
    while True:
        born, survive = int(rng.integers(0, full + 1)), int(rng.integers(0, full + 1))
        if 0 < born < full and 0 < survive < full:
            return RefRule(neighbours, born, survive, iterations, scope, outside)


def pairs_seen(world, origin, dims, rule: RefRule, mask=None) -> set:
    """the pairs (self, count) that decide some free voxel of the box in some step, by the numpy restatement"""
    r = apply_rule(world, origin, dims, rule, mask, keep_steps=True)
    seen, w = set(), r["w0"]
    for after, c in r["steps"]:
        for s in (0, 1):
            seen |= {(s, int(v)) for v in np.unique(c[r["free"] & (w == bool(s))])}
        w = after
    return seen
