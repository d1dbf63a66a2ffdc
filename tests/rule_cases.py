"""Hand-derived cases of the neighbour-count voxel rules (include/vxrt.h, vxrt_apply_rule): worlds of 64^3 voxels (the
smallest the library holds at brick edge 8) with a few solid voxels, the box, the rule, and the result worked out by hand --
the solid voxels of W_n in the box as a frozenset of world coordinates, the summary, and the packed words where a word
boundary matters.  `check` compares any implementation's result with them.
TEST INFRASTRUCTURE ONLY: imported by tests/ alone."""
from __future__ import annotations

from itertools import product

import numpy as np

from tests import ref_rule as R

EDGE = 64
NONE_MIN, NONE_MAX = (R.INT_MAX,) * 3, (R.INT_MIN,) * 3


def _world(*voxels) -> np.ndarray:
    w = np.zeros((EDGE, EDGE, EDGE), bool)
    for v in voxels:
        w[v] = True
    return w


def _case(name, world, origin, dims, rule, solid, summary, mask=None, words=None) -> dict:
    return {"name": name, "world": world, "origin": origin, "dims": dims, "rule": rule, "mask": mask, "solid": frozenset(solid),
            "summary": summary, "words": words}


def one_voxel_grows(neighbours: int) -> dict:
    """one voxel under grow: itself and its 6, 18 or 26 neighbours, the changed box one voxel around it"""
    s = (10, 10, 10)
    solid = {s} | {(s[0] + a, s[1] + b, s[2] + c) for a, b, c in R.offsets(neighbours)}
    n = {R.N6: 6, R.N18: 18, R.N26: 26}[neighbours]
    assert len(solid) == n + 1
    return _case("one voxel grows, N%d" % n, _world(s), (8, 8, 8), (5, 5, 5), R.grow(neighbours), solid,
                 (1, n + 1, n, 0, n, (9, 9, 9), (11, 11, 11)))


def cube_erodes() -> dict:
    """a 3^3 cube under erode N26: only the centre has all 26 neighbours"""
    cube = list(product(range(20, 23), repeat=3))
    return _case("cube erodes", _world(*cube), (19, 19, 19), (5, 5, 5), R.erode(R.N26), {(21, 21, 21)},
                 (27, 1, 0, 26, 26, (20, 20, 20), (22, 22, 22)))


def identity() -> dict:
    """born = none, survive = all: the box is read back as it is and the changed box is the empty pair"""
    rng = np.random.default_rng(5)
    w = rng.random((EDGE, EDGE, EDGE)) < 0.4
    o, d = (-3, 50, 7), (40, 20, 9)  # partly outside the world in x and y
    solid = {(x, y, z) for x, y, z in product(range(0, 37), range(50, 64), range(7, 16)) if w[x, y, z]}
    n = len(solid)
    return _case("identity", w, o, d, R.RefRule(R.N18, 0, (2 << 18) - 1, 3), solid, (n, n, 0, 0, 0, NONE_MIN, NONE_MAX))


def grows_across_a_word() -> dict:
    """a voxel at x = 31 of a 33-wide box grows into x = 32, the second word of its row; the padding bits stay 0"""
    o, d = (4, 8, 8), (33, 3, 3)
    s = (35, 9, 9)  # box voxel (31, 1, 1)
    solid = {s, (34, 9, 9), (36, 9, 9), (35, 8, 9), (35, 10, 9), (35, 9, 8), (35, 9, 10)}
    words = np.zeros(2 * 3 * 3, np.uint32)  # word xw + 2 * (y + 3 * z)
    words[2 * (1 + 3 * 1)] = 1 << 30 | 1 << 31
    words[2 * (1 + 3 * 1) + 1] = 1
    for y, z in ((0, 1), (2, 1), (1, 0), (1, 2)):
        words[2 * (y + 3 * z)] = 1 << 31
    return _case("grows across a word", _world(s), o, d, R.grow(R.N6), solid, (1, 7, 6, 0, 6, (34, 8, 8), (36, 10, 10)), words=words)


def on_the_worlds_face(outside: int) -> dict:
    """one voxel at x = 0, N6, born = {1, 2}, survive = {1}; the box's first column lies outside the world.
    outside = 0: the voxel has no solid neighbour and dies, its five neighbours in the world have one and are born.
    outside = 1: the column x = -1 is solid: the voxel has one solid neighbour and stays, every empty voxel of the box at
    x = 0 has one or two and is born, and so is (1, 30, 30); the column itself reads 0."""
    s = (0, 30, 30)
    rule = R.RefRule(R.N6, 0b110, 0b010, 1, R.BOX, outside)
    if outside == 0:
        solid = {(1, 30, 30), (0, 29, 30), (0, 31, 30), (0, 30, 29), (0, 30, 31)}
        summary = (1, 5, 5, 1, 6, (0, 29, 29), (1, 31, 31))
    else:
        solid = {(0, y, z) for y in (29, 30, 31) for z in (29, 30, 31)} | {(1, 30, 30)}
        summary = (1, 10, 9, 0, 9, (0, 29, 29), (1, 31, 31))
    return _case("on the world's face, outside %d" % outside, _world(s), (-1, 29, 29), (3, 3, 3), rule, solid, summary)


def beside_the_box(scope: int) -> dict:
    """a voxel two steps from the box's face, grow N6 twice.  WORLD: (20, 20, 20) is born in step 1 and (21, 20, 20), in the
    box, in step 2.  BOX: (20, 20, 20) is frozen empty and nothing in the box ever has a solid neighbour."""
    w = _world((19, 20, 20))
    rule = R.grow(R.N6, 2, scope=scope)
    if scope == R.WORLD:
        return _case("beside the box, WORLD", w, (21, 18, 18), (4, 5, 5), rule, {(21, 20, 20)},
                     (0, 1, 1, 0, 1, (21, 20, 20), (21, 20, 20)))
    return _case("beside the box, BOX", w, (21, 18, 18), (4, 5, 5), rule, set(), (0, 0, 0, 0, 0, NONE_MIN, NONE_MAX))


def half_masked() -> dict:
    """grow N6 of a voxel in the middle of the box, the voxels of box x < 2 frozen by the mask: (29, 30, 30) is not born"""
    mask = np.zeros((5, 5, 5), bool)
    mask[2:] = True
    solid = {(30, 30, 30), (31, 30, 30), (30, 29, 30), (30, 31, 30), (30, 30, 29), (30, 30, 31)}
    return _case("half masked", _world((30, 30, 30)), (28, 28, 28), (5, 5, 5), R.grow(R.N6), solid,
                 (1, 6, 5, 0, 5, (30, 29, 29), (31, 31, 31)), mask=mask)


def blinker() -> dict:
    """born = {0}, survive = none on an empty box: every voxel is born in step 1 and dies in step 2, so W_2 = W_0 while the
    last step changed all 27 voxels"""
    return _case("blinker", _world((1, 1, 1)), (40, 40, 40), (3, 3, 3), R.RefRule(R.N6, 1, 0, 2), set(),
                 (0, 0, 0, 0, 27, NONE_MIN, NONE_MAX))


def all_cases() -> list:
    return [one_voxel_grows(R.N6), one_voxel_grows(R.N18), one_voxel_grows(R.N26), cube_erodes(), identity(), grows_across_a_word(),
            on_the_worlds_face(0), on_the_worlds_face(1), beside_the_box(R.BOX), beside_the_box(R.WORLD), half_masked(), blinker()]


def gradient_cases() -> list:
    """the randomized cases in which every table entry decides some voxel (asserted on the reference alone by
    tests/test_rule_host.py): a gradient world of 64^3, random tables; (world, origin, dims, rule, mask) per case"""
    rng = np.random.default_rng(21)
    w = R.gradient_world(rng)
    cases = []
    for nb in (R.N6, R.N18, R.N26):
        cases.append((w, (0, 10, 12), (64, 20, 18), R.random_rule(rng, nb, 1, R.BOX, 0), None))
        cases.append((w, (-5, 40, -2), (74, 30, 20), R.random_rule(rng, nb, 2, R.WORLD, 1), None))
        cases.append((w, (1, 3, 30), (62, 9, 40), R.random_rule(rng, nb, 2, R.BOX, 1), rng.random((62, 9, 40)) < 0.8))
    return cases


def pack(bits: np.ndarray) -> np.ndarray:
    """bool [x, y, z] -> region words"""
    X, Y, Z = bits.shape
    rows = np.zeros((Z, Y, (X + 31) // 32 * 32), bool)
    rows[:, :, :X] = bits.transpose(2, 1, 0)
    return np.packbits(rows, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


def check(case: dict, result: dict, words=None) -> None:
    """`result`: {"bits": bool [x, y, z] of the box, "summary"}; `words`: the packed output, when the implementation has one"""
    o = case["origin"]
    assert tuple(result["bits"].shape) == tuple(case["dims"]), case["name"]
    got = frozenset((int(x) + o[0], int(y) + o[1], int(z) + o[2]) for x, y, z in np.argwhere(result["bits"]))
    assert got == case["solid"], (case["name"], sorted(got ^ case["solid"]))
    assert tuple(result["summary"]) == case["summary"], (case["name"], result["summary"])
    s = case["summary"]
    assert s[1] == s[0] + s[2] - s[3]
    if case["words"] is not None:
        have = pack(result["bits"]) if words is None else np.asarray(words).view(np.uint32)
        assert np.array_equal(have, case["words"]), case["name"]
