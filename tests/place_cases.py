"""Hand-derived cases of the voxel piece query (include/vxrt.h, vxrt_place_pieces) and of the falling-island rule, with the
expected numbers written out.  Every world is 16 x 16 x 16 with a floor; CASES rows are (name, world, piece, origin, axis,
dist, (overlap, travel, contact, flags)); DROP_CASES rows are (name, world, box origin, box dims, rows (id, voxels, travel,
contact) in dropping order).  TEST INFRASTRUCTURE ONLY: imported by tests/ alone."""
import numpy as np

BLOCKED, INVALID = 1, 2
N = 16


def floor_world(top=4):
    """solid below y = top (the floor's top face is at y = top)"""
    v = np.zeros((N, N, N), bool)
    v[:, :top, :] = True
    return v


def cube(n=2):
    return np.ones((n, n, n), bool)


def _post_world():
    v = floor_world(4)
    v[6, 4:7, 4] = True  # a post on the floor: x = 6, z = 4, top face at y = 7
    return v


def _gamma():
    """a column of three voxels with a one-voxel arm at its top: the arm's underside is the inner corner"""
    p = np.zeros((2, 3, 1), bool)
    p[0, :, 0] = True
    p[1, 2, 0] = True
    return p


def padded_words(piece):
    """the region words of a piece with every padding bit of every row's last word SET (they are not voxels)"""
    X, Y, Z = piece.shape
    wpr = (X + 31) // 32
    rows = np.ones((Z, Y, wpr * 32), bool)
    rows[:, :, :X] = piece.transpose(2, 1, 0)
    return np.packbits(rows, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


WIDE = np.ones((33, 1, 1), bool)  # one row of two words, 31 padding bits

CASES = [
    # a 2^3 cube whose underside is on the floor's top face: step 1 is blocked by its 2 x 2 footprint
    ("cube resting on the floor", floor_world(), cube(), (4, 4, 4), 1, -5, (0, 0, 4, BLOCKED)),
    # two free steps, then the footprint
    ("cube two above the floor", floor_world(), cube(), (4, 6, 4), 1, -5, (0, -2, 4, BLOCKED)),
    # column x = 5, y = 8 .. 10 (4 free steps down to the floor); arm voxel (6, 10) above the post's top voxel y = 6: 3 steps
    ("the inner corner lands first", _post_world(), _gamma(), (5, 8, 4), 1, -10, (0, -3, 1, BLOCKED)),
    # nothing solid at y >= 4: the cube leaves the world at x = 16 and keeps going
    ("out of the world", floor_world(), cube(), (4, 4, 4), 0, 20, (0, 20, 0, 0)),
    # the lower layer of the cube is inside the floor's top layer (4 voxels); upwards every step is free
    ("overlapping at the start, moving out", floor_world(), cube(), (4, 3, 4), 1, 3, (4, 3, 0, 0)),
    # downwards its first step meets the floor's layers y = 2 and 3: 8 voxels
    ("overlapping at the start, moving in", floor_world(), cube(), (4, 3, 4), 1, -2, (4, 0, 8, BLOCKED)),
    ("an empty piece", floor_world(), np.zeros((3, 3, 3), bool), (4, 2, 4), 1, -6, (0, -6, 0, 0)),
    # x = -10 .. 22 in the floor's top layer: the 16 voxels inside the world; one step up is free
    ("a 33-wide row across the world", floor_world(), WIDE, (-10, 3, 4), 1, 1, (16, 1, 0, 0)),
    # sideways inside the floor: blocked at once by the 16 voxels it would meet (x = -9 .. 23)
    ("a 33-wide row pushed along x", floor_world(), WIDE, (-10, 3, 4), 0, 7, (16, 0, 16, BLOCKED)),
    # from above the world's top: y = 20 down to the floor's top face at y = 4
    ("falling into the world from above", floor_world(), cube(), (4, 20, 4), 1, -30, (0, -16, 4, BLOCKED)),
]


def _stacked():
    v = floor_world(2)
    v[4:6, 5:7, 4:6] = True    # cube A, y = 5 .. 6: falls 3 onto the floor (top face y = 2)
    v[4:6, 9:11, 4:6] = True   # cube B, y = 9 .. 10: then falls 5 onto A (now y = 2 .. 3, top face y = 4)
    return v


def _arch():
    v = floor_world(2)
    v[6, 2:6, 4] = True        # a pillar on the floor, top voxel y = 5
    v[4, 6:8, 4] = True        # the arch: two legs y = 6 .. 7 (4 free steps to the floor) ...
    v[8, 6:8, 4] = True
    v[4:9, 8, 4] = True        # ... and a span at y = 8, whose voxel x = 6 is 2 free steps above the pillar
    return v


def island_id(x, y, z, dims=(N, N, N)):
    return 1 + x + dims[0] * (y + dims[1] * z)


DROP_CASES = [
    ("two stacked cubes", _stacked(), (0, 0, 0), (N, N, N),
     [(island_id(4, 5, 4), 8, -3, 4), (island_id(4, 9, 4), 8, -5, 4)]),
    ("an arch caught by a pillar under its span", _arch(), (0, 0, 0), (N, N, N), [(island_id(4, 6, 4), 9, -2, 1)]),
]
