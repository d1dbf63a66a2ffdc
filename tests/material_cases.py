"""The cases of the voxel-material tests (include/vxrt.h, vxrt_material_field / vxrt_material_frame), shared by the host and the
GPU tests: random leaky-terrain worlds, band sets, paint boxes, palettes and atlases that are functions of their arguments
alone, and small hand-derived scenes under axis-aligned ortho cameras whose expected bytes and colours can be written out."""
import functools

import numpy as np

from tests import light_frame_cases as LC
from tests import ref_denoise as R
from tests import ref_material as M

F32 = np.float32
WORLD = LC.WORLD  # (64, 64, 64): the smallest world the tables hold at brick edge 8
# Four bands whose edges (20, 32, 50) lie inside the field boxes below; under_depth 0 (no `under` at all) and 15 (the
# deepest walk) both occur, and every band has its own ids, so that a byte names the band and the branch that made it
RULES = ((None, 1, 2, 3, 3), (20, 4, 5, 6, 0), (32, 7, 8, 9, 15), (50, 10, 11, 12, 2))
ONE_BAND = ((None, 21, 22, 23, 1),)
PAINT_BOX = ((-3, 18, 10), (40, 30, 33))  # overlaps the world, the field boxes and the frames' hits in part
ORTHO_SIZE = (24.0, 20.0)
POSES = {  # (origin, fwd, up, right)
    "slant": ((14.5, 44.25, 20.75), (0.3, -0.9, 0.2), (0.1, 0.2, 0.95), (0.95, 0.3, -0.1)),   # looking down: tops and sides
    "up": ((30.5, 3.25, 28.75), (0.25, 0.9, 0.3), (0.1, -0.3, 0.95), (0.95, -0.2, -0.1)),      # looking up: bottoms and sides
    "axis": ((20.5, 60.0, 24.5), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),            # axis-aligned
    "zero": ((14.5, 44.25, 20.75), (0.0, 0.0, 0.0), (0.1, 0.2, 0.95), (0.95, 0.3, -0.1)),       # d = 0: the centre fallback
}
# (W, H, ortho, pose): the frames of the contract's tests in both camera kinds and under every pose
FRAME_CASES = [(1, 1, False, "slant"), (63, 5, False, "slant"), (64, 4, True, "up"), (65, 9, False, "up"), (257, 3, True, "slant"),
               (64, 4, True, "zero"), (65, 9, True, "axis"), (96, 64, False, "up"), (96, 64, True, "slant"),
               (65, 5, False, "slant")]  # partial tiles on both axes
# field boxes (origin, dims): widths 1, 31, 32, 33, 63, 64, 65 and 257 (byte and dword rows, one and several x chunks, rows
# shared by several z per wave), heights that cross a y-segment boundary and the 16-row warm-up, boxes over every face of
# the world
FIELD_BOXES = [((5, 0, 7), (1, 64, 3)), ((-4, 10, 2), (31, 45, 5)), ((16, -3, -2), (32, 70, 4)), ((40, 30, 60), (33, 40, 9)),
               ((-10, 15, 30), (63, 20, 2)), ((0, 0, 0), (64, 64, 64)), ((-1, 47, 20), (65, 30, 3)), ((-100, 12, 33), (257, 24, 2)),
               ((8, 17, 8), (12, 131, 70))]


@functools.lru_cache(maxsize=None)
def terrain_world(seed=0, shape=WORLD):
    """a height field of hills (solid below it), leaky: random holes everywhere, a cave layer, floating overhangs above the
    ground, single floating voxels, and a few columns that reach the world's top.  Read-only."""
    rng = np.random.default_rng(4242 + seed)
    X, Y, Z = shape
    x, z = np.meshgrid(np.arange(X), np.arange(Z), indexing="ij")
    height = (Y * (0.45 + 0.2 * np.sin(x / 9.0 + seed) * np.cos(z / 7.0) + 0.1 * np.sin((x + z) / 5.0))).astype(np.int64)
    y = np.arange(Y)[None, :, None]
    w = y < height[:, None, :]
    w &= rng.random(shape) > 0.04                      # leaks: runs of every length
    w[:, Y // 4:Y // 4 + 3, :] &= rng.random((X, 3, Z)) > 0.6   # a cave layer
    over = rng.random((X, Z)) < 0.08
    w[:, Y - 12:Y - 9, :] |= over[:, None, :]          # overhangs: slabs three thick above the ground
    w |= rng.random(shape) < 0.01                      # floating voxels
    for cx, cz in ((3, 3), (X - 1, Z // 2), (X // 2, 0)):
        w[cx, :, cz] = True                            # columns up to the world's top
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def paint_bytes(seed=0, box=PAINT_BOX):
    """random paint over `box`: half of it 0 (not painted), ids 100 .. 140 elsewhere; uint8 [x, y, z], read-only"""
    rng = np.random.default_rng(77 + seed)
    p = np.where(rng.random(box[1]) < 0.5, 0, rng.integers(100, 141, box[1])).astype(np.uint8)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def palette(n_tiles, seed=0):
    """tints in 0 .. 1.5 (some exactly 0 and 1), tiles drawn from 0 .. n_tiles + 1 and NO_TILE: indices at n_tiles - 1, at
    n_tiles and beyond occur for every face class"""
    rng = np.random.default_rng(555 + seed)
    tints = (rng.random((256, 3)) * 1.5).astype(F32)
    tints[::17] = 1.0
    tints[5::23] = 0.0
    tiles = rng.integers(0, n_tiles + 2, (256, 3)).astype(np.int64)
    tiles[rng.random((256, 3)) < 0.15] = M.NO_TILE
    for m, row in ((1, (n_tiles - 1, n_tiles, M.NO_TILE)), (2, (n_tiles, M.NO_TILE, n_tiles - 1)), (3, (M.NO_TILE, n_tiles - 1, n_tiles))):
        tiles[m] = row
    tints.setflags(write=False)
    tiles.setflags(write=False)
    return tints, tiles


@functools.lru_cache(maxsize=None)
def atlas(n_tiles, shift, seed=0):
    rng = np.random.default_rng(999 + 10 * shift + seed)
    a = rng.integers(0, 256, (n_tiles, 1 << shift, 1 << shift, 4), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frame_case(W, H, ortho, pose, seed=0):
    """a terrain world, a camera, colours from tests/ref_denoise.py's random frames and hit indices of five kinds: voxels on
    the pixel's own ray (the position on the face lies inside it), random voxels of the world (it is clamped), voxels on
    the world's boundary, indices outside 0 .. X*Y*Z - 1 and -1.  Everything read-only."""
    rng = np.random.default_rng(313 * W + 19 * H + 7 * seed + int(ortho) + 11 * sorted(POSES).index(pose))
    X, Y, Z = WORLD
    world = terrain_world(seed)
    color, _ = R.random_frame(W, H, seed)
    cam = tuple(np.asarray(v, F32) for v in POSES[pose])
    o, d = R.primary_rays(W, H, *cam, ortho=ortho, ortho_size=ORTHO_SIZE)
    along = (o.astype(np.float64) + rng.uniform(2.0, 40.0, (H, W, 1)) * d).astype(np.int64)
    on_ray = ((along >= 0) & (along < WORLD)).all(-1)
    along = np.clip(along, 0, np.array(WORLD) - 1)
    anywhere = np.stack([rng.integers(0, n, (H, W)) for n in WORLD], -1)
    edge = anywhere.copy()
    side = rng.integers(0, 3, (H, W))
    np.put_along_axis(edge, side[..., None], np.where(rng.random((H, W, 1)) < 0.5, 0, np.take(WORLD, side)[..., None] - 1), -1)
    index = lambda v: v[..., 0] + X * (v[..., 1] + Y * v[..., 2])
    pick = rng.random((H, W))
    hit = np.where(on_ray, index(along), index(anywhere))
    hit = np.where((pick >= 0.5) & (pick < 0.7), index(anywhere), hit)
    hit = np.where((pick >= 0.7) & (pick < 0.85), index(edge), hit)
    hit = np.where((pick >= 0.85) & (pick < 0.9), X * Y * Z + rng.integers(0, 3, (H, W)) * (1 << 40), hit)
    hit = np.where(pick >= 0.9, -1, hit).astype(np.int64)
    keys = R.keys_np(hit, WORLD, o, d)
    for a in (color, hit, keys, o, d):
        a.setflags(write=False)
    return dict(world=world, color=color, hit=hit, keys=keys, cam=cam, ortho=ortho, ortho_size=ORTHO_SIZE, o=o, d=d)


def run_frame(case, rules=RULES, shift=3, n_tiles=5, with_atlas=True, paint=True, scalar=False, told_tiles=None):
    """the restatement on a frame case -> (colour, ids, summary[, info])"""
    fn = M.material_frame_scalar if scalar else M.material_frame_np
    return fn(case["color"], case["keys"], case["hit"], case["o"], case["d"], case["world"], rules, palette(n_tiles),
              atlas(n_tiles, shift) if with_atlas else None, paint_bytes() if paint else None, PAINT_BOX, n_tiles=told_tiles)


# ---- hand-derived scenes -----------------------------------------------------------------------------------------------
# Ortho cameras along an axis over an N x N frame with the window (N / 2 / k, N / 2 / k): the ray of pixel (x, y) starts at
# pos + (x / k - N / 2 / k) * right + (y / k - N / 2 / k) * up: k pixels per voxel.
VIEWS = {  # name: (fwd, up, right)
    "down": ((0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), "upward": ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),
    "+x": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), "-x": ((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
    "+z": ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)), "-z": ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)),
}


def march_hits(world, o, d, steps=200):
    """the hit index of every ray of an axis-aligned ortho camera: the first solid voxel at floor(o + t * d), t = 0, 1, ..."""
    X, Y, Z = world.shape
    H, W = o.shape[:2]
    hit = np.full((H, W), -1, np.int64)
    for t in range(steps):
        p = np.floor(o.astype(np.float64) + t * d.astype(np.float64)).astype(np.int64)
        inside = ((p >= 0) & (p < world.shape)).all(-1)
        pc = np.clip(p, 0, np.array(world.shape) - 1)
        s = inside & world[pc[..., 0], pc[..., 1], pc[..., 2]] & (hit < 0)
        hit = np.where(s, p[..., 0] + X * (p[..., 1] + Y * p[..., 2]), hit)
    return hit


def view(world, name, pos, rules, pal, atl=None, paint=None, paint_box=None, N=8, k=1, color=0.5):
    """both restatements on the frame of camera `name` at `pos`, asserted equal -> (colour, ids, summary, info, o): o the ray
    origins (H, W, 3), which say where in the world every pixel looks"""
    cam = tuple(np.asarray(v, F32) for v in (pos, *VIEWS[name]))
    win = (N / 2.0 / k, N / 2.0 / k)
    o, d = R.primary_rays(N, N, *cam, ortho=True, ortho_size=win)
    hit = march_hits(world, o, d)
    keys = R.keys_np(hit, world.shape, o, d)
    c = np.full((N, N, 3), color, F32)
    a = M.material_frame_np(c, keys, hit, o, d, world, rules, pal, atl, paint, paint_box)
    b = M.material_frame_scalar(c, keys, hit, o, d, world, rules, pal, atl, paint, paint_box)
    assert np.array_equal(R.bits(a[0]), R.bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    return a[0], a[1], a[2], a[3], o


def plain_palette(tints=None, tiles=None):
    """white, untextured entries, then `tints` {m: (r, g, b)} and `tiles` {m: (top, side, bottom)}"""
    t = np.ones((256, 3), F32)
    s = np.full((256, 3), M.NO_TILE, np.int64)
    for m, v in (tints or {}).items():
        t[m] = v
    for m, v in (tiles or {}).items():
        s[m] = v
    return t, s
