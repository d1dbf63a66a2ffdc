"""Hand-derived cases of the voxel light field (include/vxrt.h, vxrt_light_field): worlds, boxes, emitters and the expected
sky and block levels written out with arithmetic on coordinates -- never with tests/ref_light.py.  Shared by
tests/test_light_host.py (the restatements and the host harness) and tests/test_gpu_light.py (the device).
Every world has 64 x 64 x 64 or 64 x 128 x 64 voxels: it builds with brick edge 8."""
from __future__ import annotations

import numpy as np

SKY, BLOCK = 1, 2


def _grid(origin, dims):
    """world coordinates of the voxels of B as three broadcastable arrays"""
    x, y, z = (np.arange(o, o + d) for o, d in zip(origin, dims))
    return x[:, None, None], y[None, :, None], z[None, None, :]


def _case(name, world, origin, dims, sky, block, emitters=None, counts=(0, 0, 0, 0)):
    shape = tuple(dims)
    return {"name": name, "world": world, "origin": tuple(origin), "dims": shape, "emitters": emitters,
            "sky": np.broadcast_to(np.asarray(sky, np.int64), shape), "block": np.broadcast_to(np.asarray(block, np.int64), shape),
            "counts": counts}


def open_air_over_a_floor():
    w = np.zeros((64, 64, 64), bool)
    w[:, :5, :] = True
    o, d = (10, 0, 10), (20, 30, 20)
    x, y, z = _grid(o, d)
    return _case("floor", w, o, d, np.where(y < 5, 0, 15) + 0 * x + 0 * z, 0)


def sealed_room():
    """an 11^3 room in solid rock, a level-15 emitter at its centre: sky 0, block 15 - L1 distance (the room is convex)"""
    w = np.ones((64, 64, 64), bool)
    w[20:31, 20:31, 20:31] = False
    o, d = (18, 18, 18), (15, 15, 15)
    x, y, z = _grid(o, d)
    room = (x >= 20) & (x <= 30) & (y >= 20) & (y <= 30) & (z >= 20) & (z <= 30)
    l1 = abs(x - 25) + abs(y - 25) + abs(z - 25)
    return _case("room", w, o, d, 0, np.where(room, np.maximum(15 - l1, 0), 0), [(25, 25, 25, 15)], (1, 0, 0, 0))


def shaft_into_a_corridor():
    """rock below y = 40, open air above; a 1 x 1 shaft at (10, 30 .. 39, 32) and a corridor (10 .. 40, 30, 32): 15 down the
    shaft, then 14, 13, ... along the corridor"""
    w = np.zeros((64, 64, 64), bool)
    w[:, :40, :] = True
    w[10, 30:40, 32] = False
    w[10:41, 30, 32] = False
    o, d = (8, 28, 30), (34, 14, 5)
    x, y, z = _grid(o, d)
    shaft = (x == 10) & (y >= 30) & (y < 40) & (z == 32)
    corridor = (x >= 10) & (x <= 40) & (y == 30) & (z == 32)
    sky = np.where(y >= 40, 15, np.where(shaft, 15, np.where(corridor, np.maximum(15 - (x - 10), 0), 0))) + 0 * z
    return _case("shaft", w, o, d, sky, 0)


def u_shaped_corridor():
    """solid rock with a U at y = 30: leg (10 .. 14, 30, 20), bend (14, 30, 20 .. 24), leg (14 .. 10, 30, 24); a level-15
    emitter at (10, 30, 20).  (10, 30, 24) is 4 away in L1 and 12 along the corridor: level 3, not 11"""
    w = np.ones((64, 64, 64), bool)
    w[10:15, 30, 20] = False
    w[14, 30, 20:25] = False
    w[10:15, 30, 24] = False
    o, d = (8, 28, 18), (9, 5, 9)
    x, y, z = _grid(o, d)
    in_x = (x >= 10) & (x <= 14) & (y == 30)
    block = np.where(in_x & (z == 20), 15 - (x - 10), 0)
    block = np.where((x == 14) & (y == 30) & (z > 20) & (z <= 24), 15 - 4 - (z - 20), block)
    block = np.where(in_x & (x < 14) & (z == 24), 15 - 8 - (14 - x), block)
    c = _case("u", w, o, d, 0, block, [(10, 30, 20, 15)], (1, 0, 0, 0))
    assert c["block"][2, 2, 6] == 3  # voxel (10, 30, 24)
    return c


def overhang():
    """a floor below y = 5 and a slab at y = 10 over x 20 .. 29: under it, 15 less the steps to the nearer open side, so the
    voxel under the slab's edge next to open air has 14"""
    w = np.zeros((64, 64, 64), bool)
    w[:, :5, :] = True
    w[20:30, 10, :] = True
    o, d = (15, 5, 10), (20, 5, 5)
    x, y, z = _grid(o, d)
    under = (x >= 20) & (x < 30)
    sky = np.where(under, 15 - np.minimum(x - 19, 30 - x), 15) + 0 * y + 0 * z
    c = _case("overhang", w, o, d, sky, 0)
    assert c["sky"][5, 2, 0] == 14 and c["sky"][4, 2, 0] == 15
    return c


def sky_hole_outside_the_box(distance):
    """rock below y = 50; a shaft at x = 10 from y = 30 to the open air and a sealed corridor (10 .. 40, 30, 32); B is the five
    corridor voxels from x = 10 + distance: the hole `distance` = 14 voxels outside B gives 1 on the nearest, 15 gives 0"""
    w = np.zeros((64, 64, 64), bool)
    w[:, :50, :] = True
    w[10, 30:50, 32] = False
    w[10:41, 30, 32] = False
    o, d = (10 + distance, 30, 32), (5, 1, 1)
    x, y, z = _grid(o, d)
    return _case("hole%d" % distance, w, o, d, np.maximum(15 - (x - 10), 0) + 0 * y + 0 * z, 0)


def emitter_classes():
    """the sealed room with entries of every class: two on the centre (levels 7 and 12: 12 counts), a level-1 emitter in a
    corner 15 steps from the centre (it lights only its own voxel), one in rock, one far away, two invalid levels"""
    w = np.ones((64, 64, 64), bool)
    w[20:31, 20:31, 20:31] = False
    o, d = (18, 18, 18), (15, 15, 15)
    x, y, z = _grid(o, d)
    room = (x >= 20) & (x <= 30) & (y >= 20) & (y <= 30) & (z >= 20) & (z <= 30)
    l1 = abs(x - 25) + abs(y - 25) + abs(z - 25)
    block = np.where(room, np.maximum(12 - l1, 0), 0)
    block = np.where((x == 20) & (y == 20) & (z == 20), 1, block)
    e = [(25, 25, 25, 7), (10, 10, 10, 9), (25, 25, 25, 12), (20, 20, 20, 1), (25, 25, 25, 0), (60, 60, 60, 5), (25, 25, 25, 16),
         (25, 25, 25, 7)]
    return _case("classes", w, o, d, 0, block, e, (4, 1, 1, 2))


def box_outside_the_world():
    w = np.ones((64, 64, 64), bool)
    return _case("outside", w, (200, -50, 300), (5, 4, 3), 15, 0)


def plate_above_the_halo():
    """a floor below y = 5 and a plate at y = 120 over x, z 20 .. 29, far above the halo's top row (y = 24): the columns under
    it are not exposed, and have 15 less the steps to the nearest column that is.  A halo-only implementation gives 15"""
    w = np.zeros((64, 128, 64), bool)
    w[:, :5, :] = True
    w[20:30, 120, 20:30] = True
    o, d = (15, 5, 15), (20, 6, 20)
    x, y, z = _grid(o, d)
    under = (x >= 20) & (x < 30) & (z >= 20) & (z < 30)
    steps = np.minimum(np.minimum(x - 19, 30 - x), np.minimum(z - 19, 30 - z))
    c = _case("plate", w, o, d, np.where(under, 15 - steps, 15) + 0 * y, 0)
    assert c["sky"][9, 0, 9] == 10
    return c


def all_cases():
    return [open_air_over_a_floor(), sealed_room(), shaft_into_a_corridor(), u_shaped_corridor(), overhang(),
            sky_hole_outside_the_box(14), sky_hole_outside_the_box(15), emitter_classes(), box_outside_the_world(),
            plate_above_the_halo()]


def check(case, result, channels=SKY | BLOCK):
    """`result` (levels [x, y, z] and a summary in tests/ref_light.py's form) against the case's expected arrays"""
    sky = case["sky"] if channels & SKY else np.zeros(case["dims"], np.int64)
    block = case["block"] if channels & BLOCK else np.zeros(case["dims"], np.int64)
    want = (sky << 4 | block).astype(np.uint8)
    assert np.array_equal(result["levels"], want), (case["name"], channels)
    s = result["summary"]
    assert (s[4], s[5]) == (int(sky.sum()), int(block.sum())), (case["name"], channels)
    assert tuple(s[6:10]) == (tuple(case["counts"]) if channels & BLOCK else (0, 0, 0, 0)), (case["name"], channels)
    o, d = case["origin"], case["dims"]
    x, y, z = _grid(o, d)
    X, Y, Z = case["world"].shape
    inside = (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
    solid = np.zeros(d, bool)
    if inside.any():
        solid[inside] = case["world"][np.broadcast_to(x, d)[inside], np.broadcast_to(y, d)[inside], np.broadcast_to(z, d)[inside]]
    assert s[0] == int(solid.sum()) and sum(s[2]) == sum(s[3]) == solid.size - s[0], case["name"]
