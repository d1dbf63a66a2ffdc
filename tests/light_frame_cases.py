"""The cases of the light-on-frames tests (include/vxrt.h, vxrt_light_frame), shared by the host and the GPU tests: random
cases that are functions of their arguments alone, and hand-derived cases on small scenes with an axis-aligned ortho camera
whose window makes one pixel one voxel, so that every expected number can be written out."""
import numpy as np

from tests import ref_denoise as R
from tests import ref_light_frame as LF

F32 = np.float32
WORLD = (64, 64, 64)            # the smallest world the tables hold at brick edge 8
BOX = ((-5, 20, 8), (40, 30, 37))  # smaller than the world, partly at negative coordinates
ORTHO_SIZE = (24.0, 20.0)
PARAMS = dict(outside_level=0xC3, sky_floor=0.25, block_color=(1.0, 0.75, 0.5), ao_curve=(0.35, 0.55, 0.8, 1.0))
FLAG_SETS = (LF.SMOOTH | LF.OCCLUSION, LF.SMOOTH, LF.OCCLUSION, 0)
# (W, H, ortho, pose): the frames of the contract's tests in both camera kinds, and one frame under a camera whose forward
# vector is zero -- an ortho ray with d = 0 on every axis: the centre of the face
CASES = [(W, H, ortho, "slant") for W, H in ((67, 35), (64, 1), (1, 64), (160, 96)) for ortho in (False, True)] + [(64, 1, True, "zero")]
# one pixel (fifteen of the counting workgroup's sixteen waves walk no tile) and partial tiles on both axes
CASES += [(1, 1, False, "slant"), (65, 5, False, "slant")]


def random_case(W, H, ortho, pose="slant", seed=0):
    """a random world of density 0.35, random level bytes over BOX (not a light field), a camera inside the world looking
    down at a slant, and hit indices of five kinds: voxels on the pixel's own ray (the position on the face lies inside
    it), random voxels of the world (it is clamped), voxels on the world's boundary (front cells outside the world), indices
    outside 0 .. X*Y*Z - 1 and -1; colours from tests/ref_denoise.py's random frames.  Everything read-only."""
    rng = np.random.default_rng(991 * W + 17 * H + 5 * seed + int(ortho) + (3 if pose == "zero" else 0))
    X, Y, Z = WORLD
    world = rng.random(WORLD) < 0.35
    levels = rng.integers(0, 256, BOX[1], dtype=np.uint8)
    color, _ = R.random_frame(W, H, seed)
    fwd = (0.0, 0.0, 0.0) if pose == "zero" else (0.3, -0.9, 0.2)
    cam = tuple(np.asarray(v, F32) for v in ((14.5, 44.25, 20.75), fwd, (0.1, 0.2, 0.95), (0.95, 0.3, -0.1)))
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
    for a in (world, levels, color, hit, keys):
        a.setflags(write=False)
    return dict(world=world, levels=levels, box=BOX, color=color, hit=hit, keys=keys, cam=cam, ortho=ortho, ortho_size=ORTHO_SIZE,
                params=dict(PARAMS))


def run_case(case, flags=LF.SMOOTH | LF.OCCLUSION, scalar=False, levels=True):
    return LF.light_frame(case["color"], case["hit"], case["cam"], case["world"], case["levels"] if levels else None, case["box"],
                          dict(case["params"], flags=flags), case["ortho"], ortho_size=case["ortho_size"], scalar=scalar, keys=case["keys"])


# ---- hand-derived scenes -----------------------------------------------------------------------------------------------
# An ortho camera looking down -y with right = +x and up = +z over a W x H = 8 x 8 frame and the window (4, 4): the ray of
# pixel (x, y) starts at pos + ((x / 8) * 2 - 1) * 4 * (8 / 8), 0, ((y / 8) * 2 - 1) * 4) = pos + (x - 4, 0, y - 4): one pixel
# is one voxel.  With pos = (4.5, 40, 4.5) pixel (x, y) looks down the middle of the column (x, ., y): u = w = 0.5 on every
# top face, so a pixel's value is the plain average of its four corners.
HW = HH = 8
WINDOW = (4.0, 4.0)
DOWN, UPZ, RIGHTX = (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
FLOOR_Y = 10  # the plate's voxels: y = FLOOR_Y; its top faces: the plane y = FLOOR_Y + 1, the front cells y = FLOOR_Y + 1


def top_camera(dx=0.0, dz=0.0):
    return ((4.5 + dx, 40.0, 4.5 + dz), DOWN, UPZ, RIGHTX)


def plate_world(extra=()):
    """a plate over the whole world at y = FLOOR_Y, and the voxels of `extra`"""
    w = np.zeros(WORLD, bool)
    w[:, FLOOR_Y, :] = True
    for x, y, z in extra:
        w[x, y, z] = True
    return w


def top_hits(world):
    """the hit index of every pixel of the top camera: the highest solid voxel of column (x, ., y)"""
    X, Y, Z = world.shape
    hit = np.empty((HH, HW), np.int64)
    for py in range(HH):
        for px in range(HW):
            ys = np.flatnonzero(world[px, :, py])
            hit[py, px] = px + X * (int(ys[-1]) + Y * py) if len(ys) else -1
    return hit


def lit_from_above(world, levels=None, box=((0, 0, 0), (1, 1, 1)), params=None, cam=None, color=0.5):
    """both restatements on the top camera's frame of `world`, asserted equal -> (colour, terms, summary, info)"""
    c = np.full((HH, HW, 3), color, F32)
    hit = top_hits(world)
    kw = dict(ortho=True, ortho_size=WINDOW)
    a = LF.light_frame(c, hit, cam or top_camera(), world, levels, box, params, **kw)
    b = LF.light_frame(c, hit, cam or top_camera(), world, levels, box, params, scalar=True, **kw)
    assert np.array_equal(R.bits(a[0]), R.bits(b[0])) and np.array_equal(R.bits(a[1]), R.bits(b[1])) and a[2] == b[2]
    return a
