"""Inputs shared by the reference pin: tests/test_reference_pin.py (reference against oracle, CPU), tests/test_ref_golden.py
(recorded reference results against oracle and HIP), tests/test_gpu_reference_parity.py (reference against HIP) and the
fixture generator tests/golden/make_ref_golden.py.  Everything is rebuilt from seeds; nothing here needs the reference.

Worlds are those of tests/render_edge_cases.world (same seeds), the terrain cut to 256^3 because reference-built worlds
stay at or below 256^3 (oracle/vxref.py).  The ray seeds are the defaults of the helpers they come from.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from tests import helpers, quirk_cases, render_edge_cases as rec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_STEPS = (2048, 100, 8, 1)
FRAME_W, FRAME_H = 96, 64
FRAME_NUMBERS = (0, 1)
FRAME_WORLDS = ("terrain32", "random16")
SWITCHES = ("mode", "checkerboard", "shadow", "bounce_samples", "ortho")

# name -> (dims, brick edge); the four trace worlds of the pin
WORLDS = {"random8": ((64, 64, 64), 8), "dense8": ((64, 64, 64), 8), "random16": ((128, 128, 128), 16),
          "terrain32": ((256, 256, 256), 32)}
GOLDEN_RAY_WORLDS = ("random8", "dense8", "random16")        # "three small worlds"
GOLDEN_BUILDER_WORLDS = {8: "random8", 16: "random16", 32: "terrain32"}
GOLDEN_RAYS, GOLDEN_MAX_STEPS = 2048, (2048, 8)


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


@functools.lru_cache(maxsize=None)
def dense(name):
    """dense tiled-linear bit words of a world (read-only)"""
    from oracle import vxo
    (X, Y, Z), _ = WORLDS[name]
    if name == "terrain32":
        w = helpers.gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    else:
        density, seed = dict(random8=(0.03, 42), dense8=(0.6, 43), random16=(0.004, 41))[name]
        v = np.random.default_rng(seed).random((X, Y, Z)) < density
        if name == "dense8":
            v[28:36, 28:36, 28:36] = True
        w = vxo.dense_from_voxels(v)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def oracle_world(name):
    from oracle import vxo
    (X, Y, Z), f = WORLDS[name]
    return vxo.World.from_dense(dense(name), X, Y, Z, f)


@functools.lru_cache(maxsize=None)
def reference_world(name, variant):
    from oracle import vxref
    (X, Y, Z), f = WORLDS[name]
    return vxref.World(dense(name), X, Y, Z, f, variant)


@functools.lru_cache(maxsize=None)
def adversarial_rays(dims):
    """the 3000 rays of test_oracle_quirk_kat.test_two_restatements_agree_and_cover_every_quirk (2 x 1500, seeds 10 and 11)"""
    a, b = helpers.mixed_rays(dims, 1500, seed=10), helpers.mixed_rays(dims, 1500, seed=11)
    return _frozen(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))


@functools.lru_cache(maxsize=None)
def mixed_rays(dims, n=100000):
    return _frozen(*helpers.mixed_rays(dims, n))


def _frozen(o, d):
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def golden_rays(name):
    return mixed_rays(WORLDS[name][0], GOLDEN_RAYS)


def quirk_inputs():
    """name -> (voxels bool [x,y,z], factor, origin, dir, max_steps) of every tests/quirk_cases case"""
    out = {}
    for name, case in quirk_cases.all_cases().items():
        if "voxels" in case:
            v = np.zeros(case["size"], bool)
            for p in case["voxels"]:
                v[p] = True
            o, d = np.array(case["origin"], np.float32), np.array(case["dir"], np.float32)
        else:
            v = np.random.default_rng(case["world_seed"]).random(case["size"]) < case["density"]
            o = np.array(case["origin_bits"], np.uint32).view(np.float32)
            d = np.array(case["dir_bits"], np.uint32).view(np.float32)
        out[name] = (v, case["factor"], o, d, case["max_steps"])
    return out


def aabb_cases(n=100000, seed=0):
    """n random ray / box cases (start, dir, bmin, bmax): boxes of brick-extent shape (multiples of 1/8 inside a cell),
    starts inside, outside, on box planes; directions with zero, tiny and denormal components"""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, 16, (n, 3)).astype(np.float32)
    lo = rng.integers(0, 8, (n, 3))
    hi = np.minimum(lo + rng.integers(0, 8, (n, 3)), 7)
    bmin = cell + lo.astype(np.float32) / np.float32(8)
    bmax = cell + (hi + 1).astype(np.float32) / np.float32(8)
    s = (rng.random((n, 3)) * 18 - 1).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    i = np.arange(n)
    m = i % 2 == 0                                                 # half of the rays are aimed at (or near) their box
    c, half = (bmin + bmax) / np.float32(2), (bmax - bmin) / np.float32(2)
    d[m] = (c[m] + rng.normal(size=(int(m.sum()), 3)).astype(np.float32) * half[m] * np.float32(0.7)) - s[m]
    m = i % 3 == 0
    s[m] = np.floor(s[m] * 8) / np.float32(8)                      # on the 1/8 lattice the box planes lie on
    m = i % 5 == 0
    s[m, (i[m] // 5) % 3] = bmin[m, (i[m] // 5) % 3]               # exactly on a near plane
    m = i % 7 == 0
    d[m, (i[m] // 7) % 3] = 0
    m = i % 11 == 0
    d[m, (i[m] // 11) % 3] *= np.float32(1e-30)
    m = i % 13 == 0
    d[m, (i[m] // 13) % 3] = np.float32(1e-42)
    m = i % 17 == 0
    d[m] = -np.abs(d[m])
    m = i % 19 == 0                                                # axis-aligned
    ax = (i[m] // 19) % 3
    d[m] = 0
    d[m, ax] = np.where(i[m] & 1, 1.0, -1.0).astype(np.float32)
    m = i % 23 == 0
    s[m] = -s[m] * np.float32(0)                                   # +-0 starts
    return s, d, bmin, bmax


@functools.lru_cache(maxsize=None)
def builder_worlds():
    """name -> (voxels bool [x,y,z], brick edge): random, empty and full grids at every brick edge, and a non-cubic one"""
    rng = np.random.default_rng(7)
    out = {}
    for f in (8, 16, 32):
        n = 8 * f                               # the tiled layout wants coarse dimensions that are multiples of 8
        out["random_f%d" % f] = (rng.random((n, n, n)) < 0.3 / f ** 2, f)
        out["empty_f%d" % f] = (np.zeros((n, n, n), bool), f)
        out["full_f%d" % f] = (np.ones((n, n, n), bool), f)
    out["noncubic_f8"] = (rng.random((64, 128, 256)) < 0.003, 8)
    return out


DDA_REGION_FRACTION = 0.75


def dda_region(dims):
    """the region of the single-level traversal's region-check runs: three quarters of the grid along x"""
    return (0.0, 0.0, 0.0, dims[0] * DDA_REGION_FRACTION + 0.9, float(dims[1]), float(dims[2]))


def hash_seeds():
    """2^24 seeds in a stride across all 2^32, and the ends of the range"""
    stride = np.arange(1 << 24, dtype=np.uint64) * np.uint64(257) + np.uint64(12345)
    edge = np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64)
    return np.concatenate([stride, edge]).astype(np.uint32)


def fbm_points():
    """100k points: the range the world generator samples (0.005 * voxel), a wider one, and lattice points"""
    rng = np.random.default_rng(3)
    return np.concatenate([rng.random((60000, 3)) * 1.3, rng.random((30000, 3)) * 40.0,
                           np.floor(rng.random((10000, 3)) * 8)]).astype(np.float32)


def quirk_aabb_cases():
    """the world-entry slab test of every quirk case, as Raytrace sets it up (coarse start, unit direction, the box
    [1e-6, dims - 1e-6] with the double epsilon rounded to binary32 once)"""
    S, D, LO, HI = [], [], [], []
    for v, f, o, d, _ in quirk_inputs().values():
        with np.errstate(all="ignore"):
            unit = d * (np.float32(1) / np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), dtype=np.float32))
        S.append(o / np.float32(f))
        D.append(unit.astype(np.float32))
        LO.append(np.full(3, np.float32(1e-6), np.float32))
        HI.append(np.array([np.float32(np.float64(c // f) - 1e-6) for c in v.shape], np.float32))
    return tuple(np.array(a, np.float32) for a in (S, D, LO, HI))


# ---- frames
def frame_camera(cam, dims):
    from oracle import vxo
    return helpers.camera(cam, dims, vxo)


def make_params(W, H, camera, variant_switches, frame_number, **kw):
    """oracle.vxo.make_params for a reference variant's switches"""
    from oracle import vxo
    return vxo.make_params(W, H, *camera, frame_number=frame_number, **dict(variant_switches, **kw))


# the world a render edge case runs on here.  Reference-built worlds stay at or below 256^3, so the terrain cases run on the
# 256^3 terrain with their camera's x and z halved (the cases were written for 512 x 256 x 512: the camera keeps its place
# relative to the world, integer and half-integer coordinates stay on the lattice they were on, -0.0 stays -0.0), and the
# 65536-wide grid is left out.  test_reference_pin.test_render_edge_cases asserts that every case still reaches the
# branches it names.
WORLD_OF_CASE = {"terrain32": "terrain32", "random16": "random16", "random8": "random8", "dense8": "dense8", "wide8": None}


def variant_of_case(case, variants):
    """the reference variant (name -> switches) that can express a render edge case, or None.  Compile-time switches must
    agree: debug view, ortho, shadow trace and bounce sample count.  The checkerboard switch only chooses WHICH pixels a frame computes, so the
    case runs with the variant's setting on both sides, over two consecutive frame numbers, which computes every pixel.
    The extension flags (bounce_depth=2, bounce_all_hits=1) are dropped on both sides."""
    if WORLD_OF_CASE[case.world] is None:
        return None
    kw = case.render_kw()
    want = dict(mode=kw.get("mode", 0), shadow=kw.get("shadow", 0), bounce_samples=kw.get("bounce_samples", 0), ortho=kw.get("ortho", 0))
    if want["mode"] == 1:                                      # the debug view shades nothing
        want.update(shadow=0, bounce_samples=0)
    for name, sw in variants.items():
        if all(sw.get(k, 0) == v for k, v in want.items()):
            return name
    return None


# fov_tiny and fov_1 look along -z at y = 180 and, at half the distance, meet no terrain that high (the 256^3 terrain
# reaches 165 on their line): they look from y = 150 here
CASE_HEIGHT = {"fov_tiny": 150.0, "fov_1": 150.0}


def case_camera(case):
    """(origin, fwd, up, right) of an edge case on the world it runs on here"""
    pos, fwd, up, right = case.camera
    if case.world == "terrain32":
        pos = (float(np.float32(pos[0]) / np.float32(2)), CASE_HEIGHT.get(case.name, pos[1]), float(np.float32(pos[2]) / np.float32(2)))
    return pos, fwd, up, right


def case_params(case, variant_switches, frame_number):
    """the oracle's RenderParams of an edge case under a variant: extension flags dropped, the variant's checkerboard"""
    kw = case.render_kw()
    kw.update(bounce_depth=1, bounce_all_hits=0, checkerboard=variant_switches.get("checkerboard", 0), frame_number=frame_number)
    from oracle import vxo
    return vxo.make_params(case.W, case.H, *case_camera(case), **kw)


# ---- job files of oracle/ref_main.cpp (the reference driver under -fsanitize=float-cast-overflow)
class Job:
    def __init__(self, path):
        self.f = open(path, "wb")

    def _w(self, *arrays):
        for a in arrays:
            self.f.write(np.ascontiguousarray(a).tobytes())

    def world(self, name):
        (X, Y, Z), f = WORLDS[name]
        self.world_dense(dense(name), X, Y, Z, f)

    def world_dense(self, words, X, Y, Z, f):
        self._w(np.array([1, X, Y, Z, f], np.int32), np.asarray(words, np.uint32))

    def rays(self, o, d, max_steps):
        self._w(np.array([2, len(o), max_steps], np.int32), np.asarray(o, np.float32), np.asarray(d, np.float32))

    def frame(self, W, H, frame_number, p):
        """p: an oracle RenderParams (camera, FOV, ortho size, environment)"""
        fl = [p.fov_deg, *p.ortho_size, *p.origin, *p.fwd, *p.up, *p.right, *p.env.light_dir, *p.env.light_color, *p.env.ambient]
        self._w(np.array([3, W, H, frame_number], np.int32), np.array(fl, np.float32))

    def aabb(self, s, d, lo, hi):
        self._w(np.array([4, len(s)], np.int32), np.concatenate([s, d, lo, hi], axis=1).astype(np.float32))

    def seeds(self, seeds):
        self._w(np.array([5, len(seeds)], np.int32), np.asarray(seeds, np.uint32))

    def fbm(self, xyz):
        self._w(np.array([6, len(xyz)], np.int32), np.asarray(xyz, np.float32))

    def dda(self, words, dims, s, d, max_steps, region=None, take_initial_step=False, cell_boxes=None, scale=0):
        self._w(np.array([7, *dims, len(s), max_steps, int(region is not None), int(take_initial_step), scale if cell_boxes is not None else 0],
                         np.int32), np.asarray(words, np.uint32))
        if cell_boxes is not None:
            self._w(np.asarray(cell_boxes, np.float32))
        if region is not None:
            self._w(np.asarray(region, np.float32))
        self._w(np.asarray(s, np.float32), np.asarray(d, np.float32))

    def populate(self, X, Y, Z):
        self._w(np.array([8, X, Y, Z], np.int32))

    def close(self):
        self._w(np.array([0], np.int32))
        self.f.close()
