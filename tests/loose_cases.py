"""Cases of the loose voxels (include/vxrt.h, vxrt_loose_step) shared by the CPU and the GPU tests: hand-derived scenes with
their expected layers written out, and random scenes.  A case is a dict: world (bool [x, y, z], every axis a multiple of 64),
origin, dims, loose (bool grid of dims), material, steps, edge, phase, and for the hand-derived ones `voxels` (the expected
layer as world coordinates) and `summary`; `padding`: the input words carry set padding bits.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from tests import ref_loose as R

NONE = R.NONE


def _world(shape=(64, 64, 64), floor=True, solids=()):
    w = np.zeros(shape, bool)
    if floor:
        w[:, 0, :] = True
    for p in solids:
        w[p] = True
    return w


def _layer(origin, dims, voxels):
    g = np.zeros(dims, bool)
    for p in voxels:
        g[tuple(a - b for a, b in zip(p, origin))] = True
    return g


def _case(name, world, origin, dims, voxels_in, material, steps, edge, phase, voxels, summary, padding=False):
    return dict(name=name, world=world, origin=origin, dims=dims, loose=_layer(origin, dims, voxels_in), material=material, steps=steps,
                edge=edge, phase=phase, voxels=sorted(voxels), summary=summary, padding=padding)


def hand_cases() -> list:
    S, Wt, WALL, OPEN = R.SAND, R.WATER, R.WALL, R.OPEN
    whole = ((0, 0, 0), (8, 8, 8))  # (a corner of the 64^3 world: its +x, +y, +z faces are walls)
    cases = []
    # a single voxel falls one cell per step: from y = 4 onto the floor (y = 0) in three steps; the fourth moves nothing.  At
    # rest it cannot slide: the voxel beside and below is the floor
    for steps, fell in ((1, 1), (3, 1), (4, 0)):
        y = max(4 - steps, 1)
        cases.append(_case("fall%d" % steps, _world(), *whole, [(3, 4, 3)], S, steps, WALL, 0, [(3, y, 3)],
                           (1, 1, 1, fell, 0, 0, (3, y, 3), (3, 4, 3))))
    # a column of four in an empty world, in a walled box (1, 1, 1) + (5, 5, 5) whose floor is the box's own bottom face.
    # Step 0 (x axis; s = (z + y) & 1 = y & 1 for z = 3 ... so y = 2 and 4 go towards -x, y = 3 towards +x): the voxel at y = 1
    # stays, (3, 2, 3) -> (2, 1, 3), (3, 3, 3) -> (4, 2, 3), (3, 4, 3) -> (2, 3, 3).  Step 1 (z axis): (2, 3, 3) falls to
    # (2, 2, 3) and (4, 2, 3) to (4, 1, 3); then (2, 2, 3), resting on (2, 1, 3), has s = (x + y) & 1 = 0: towards +z, to
    # (2, 1, 4).  Step 2 moves nothing: every voxel lies on the box's floor
    col = [(3, y, 3) for y in (1, 2, 3, 4)]
    cases.append(_case("column_sand", _world(floor=False), (1, 1, 1), (5, 5, 5), col, S, 3, WALL, 0,
                       [(2, 1, 3), (2, 1, 4), (3, 1, 3), (4, 1, 3)], (4, 4, 4, 0, 0, 0, (2, 1, 3), (4, 4, 4))))
    # the same column as water, eight steps: all four on the floor and still spreading (spread_last > 0, fell = slid = 0)
    cases.append(_case("column_water", _world(floor=False), (1, 1, 1), (5, 5, 5), col, Wt, 8, WALL, 0,
                       [(3, 1, 1), (4, 1, 3), (5, 1, 1), (5, 1, 3)], (4, 4, 4, 0, 0, 3, (3, 1, 1), (5, 4, 3))))
    # a voxel one above the world's bottom face, the box open: step 0 falls to y = 0, step 1 into the sink below the world
    cases.append(_case("drain1", _world(floor=False), (2, 0, 2), (3, 3, 3), [(3, 1, 3)], S, 1, OPEN, 0, [(3, 0, 3)],
                       (1, 1, 1, 1, 0, 0, (3, 0, 3), (3, 1, 3))))
    cases.append(_case("drain2", _world(floor=False), (2, 0, 2), (3, 3, 3), [(3, 1, 3)], S, 2, OPEN, 0, [],
                       (1, 1, 0, 1, 0, 0, (3, 1, 3), (3, 1, 3))))
    # the same box walled: the voxel stays on the box's bottom face
    cases.append(_case("walled", _world(floor=False), (2, 0, 2), (3, 3, 3), [(3, 1, 3)], S, 2, WALL, 0, [(3, 0, 3)],
                       (1, 1, 1, 0, 0, 0, (3, 0, 3), (3, 1, 3))))
    # A on a ledge (3, 1, 3): s = (z + y) & 1 = 1, towards -x; (2, 2, 3) is free, (2, 1, 3) below it as well: A slides
    ledge = _world(solids=[(3, 1, 3)])
    cases.append(_case("ledge_free", ledge, *whole, [(3, 2, 3)], S, 1, WALL, 0, [(2, 1, 3)], (1, 1, 1, 0, 1, 0, (2, 1, 3), (3, 2, 3))))
    # ... and with B on (2, 1, 3) the slide target is taken.  B rests on the floor; its own direction is +x, into the ledge
    cases.append(_case("ledge_taken", ledge, *whole, [(3, 2, 3), (2, 1, 3)], S, 1, WALL, 0, [(2, 1, 3), (3, 2, 3)],
                       (2, 2, 2, 0, 0, 0, *NONE)))
    # input bits outside the world (x = -2), on a solid (the floor) and, in the words, in the padding: dropped.  The one kept
    # rests on the floor.  changed box: the two dropped bits
    cases.append(_case("dropped", _world(), (-2, 0, 0), (6, 3, 3), [(-2, 1, 1), (1, 0, 1), (2, 1, 1)], S, 1, WALL, 0, [(2, 1, 1)],
                       (3, 1, 1, 0, 0, 0, (-2, 0, 1), (1, 1, 1)), padding=True))
    # across the word boundary of a 64-wide box, both ways: water on the floor at (x, 1, 3) spreads towards +x in step 0
    # (s = (3 + 1 + 0) & 1 = 0) and towards -x in step 2; sand on a pillar (x, 1, 3) slides from (x, 2, 3) towards -x in step 0
    # (s = (3 + 2) & 1 = 1) and towards +x in step 2.  x = 30, 31, 32, 33: the boundary of the box's words (31 | 32) and of the
    # halo's, which sit one bit further (30 | 31)
    wide = ((0, 0, 0), (64, 8, 8))
    for x in (30, 31, 32, 33):
        for phase, sign in ((0, 1), (2, -1)):
            cases.append(_case("spread_x%d_t%d" % (x, phase), _world((64, 64, 64)), *wide, [(x, 1, 3)], Wt, 1, WALL, phase, [(x + sign, 1, 3)],
                               (1, 1, 1, 0, 0, 1, (min(x, x + sign), 1, 3), (max(x, x + sign), 1, 3))))
            cases.append(_case("slide_x%d_t%d" % (x, phase), _world((64, 64, 64), solids=[(x, 1, 3)]), *wide, [(x, 2, 3)], S, 1, WALL, phase,
                               [(x - sign, 1, 3)], (1, 1, 1, 0, 1, 0, (min(x, x - sign), 1, 3), (max(x, x - sign), 2, 3))))
    # every phase & 3: a lone water voxel at (3, 1, 3) on the floor goes +x, +z, -x, -z; phase + 4 and 2^32 - 4 + phase the same
    for phase, target in enumerate([(4, 1, 3), (3, 1, 4), (2, 1, 3), (3, 1, 2)]):
        for ph in (phase, phase + 4, 2 ** 32 - 4 + phase):
            cases.append(_case("phase%d" % ph, _world(), *whole, [(3, 1, 3)], Wt, 1, WALL, ph, [target],
                               (1, 1, 1, 0, 0, 1, tuple(min(a, b) for a, b in zip(target, (3, 1, 3))),
                                tuple(max(a, b) for a, b in zip(target, (3, 1, 3))))))
    # the step's number wraps: two steps from phase 2^32 - 1 are steps 2^32 - 1 (-z) and 0 (at (3, 1, 2): s = (2 + 1) & 1, -x)
    cases.append(_case("wrap", _world(), *whole, [(3, 1, 3)], Wt, 2, WALL, 2 ** 32 - 1, [(2, 1, 2)], (1, 1, 1, 0, 0, 1, (2, 1, 2), (3, 1, 3))))
    return cases


def check(case, got) -> None:
    """`got`: {"bits": bool grid of dims, "summary": tuple} against the case's written-out expectation"""
    want = _layer(case["origin"], case["dims"], case["voxels"])
    assert np.array_equal(np.asarray(got["bits"], bool), want), (case["name"], sorted(map(tuple, np.argwhere(got["bits"]).tolist())))
    assert tuple(got["summary"]) == case["summary"], (case["name"], got["summary"])


def words_of(case) -> np.ndarray:
    """the input layer as region words (uint32); with `padding` every padding bit set"""
    d = case["dims"]
    wpr = (d[0] + 31) // 32
    rows = np.zeros((d[2], d[1], wpr * 32), bool)
    rows[:, :, :d[0]] = np.asarray(case["loose"], bool).transpose(2, 1, 0)
    if case.get("padding"):
        rows[:, :, d[0]:] = True
    return np.packbits(rows, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


def random_cases(seed=0, n=12, shape=(64, 64, 64)) -> list:
    """leaky terrain, boxes inside, over the faces and outside the world, both materials and edges, steps 1 .. 5, any phase"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        world = R.terrain(rng, shape, 1, 5, 0.15)
        d = tuple(int(v) for v in rng.integers(1, 20, 3))
        o = (int(rng.integers(-4, shape[0] - 2)), int(rng.integers(-4, 5)), int(rng.integers(-4, shape[2] - 2)))
        out.append(dict(name="random%d" % i, world=world, origin=o, dims=d, loose=R.random_layer(rng, d, 0.25), material=i & 1,
                        steps=int(rng.integers(1, 6)), edge=(i >> 1) & 1, phase=int(rng.integers(0, 2 ** 32)), padding=bool(i % 3 == 0)))
    return out


def run(fn, case) -> dict:
    return fn(case["world"], case["origin"], case["dims"], case["loose"], case["material"], case["steps"], case["edge"], case["phase"])
