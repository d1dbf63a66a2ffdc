"""Field limit cases: calls of vxrt_light_field and vxrt_place_pieces whose shapes reach the code that only runs past a launch
cap.  Shared by tests/test_field_limits_host.py, which holds every case to the cap it must exceed and every construction and
closed form below to the restatements (tests/ref_light.py, tests/ref_place.py) and the host harnesses, and
tests/test_gpu_field_limits.py, which runs them on the device.

The caps live in voxelengine_amd/csrc; read_caps() reads them with regexes that must match exactly once:
- k_light_classify / k_light_scatter run one 256-lane workgroup per 256 emitters, up to kLightMaxEmitters (vxrt_light.hip);
- k_light_tally grid-strides over nt words with `few` workgroups: min(tb, 128) while tb / 8 < 128, else min(tb / 8, 1024),
  tb = ceil(nt / 256): a second pass of the loop takes nt > 128 * 256 words, the 1024 cap tb / 8 > 1024;
- light_expand_lane stores bytes when the output is not on a dword boundary (LightArgs::wide == 0; no constant);
- k_light_above takes one lane per slab of kLightSlab rows from light_above_first (the halo's top, kLightHalo over the box,
  clamped to row 0) to the world's top;
- kLightMaxVoxels voxels is the largest box;
- place_shape sizes every placement of a batch by the table's piece with the most rows (at most kPlaceMaxDim^2 of them);
  place_pieces cuts a batch into launches of at most 1 << 30 lanes, grid_2d (vxrt_region.hpp) takes a launch to a second grid
  axis past (1 << 20) workgroups, and k_place_init / k_place_finish grid-stride past 65536 workgroups (place_blocks).
Every case names the cap it must exceed.

Not covered: grid_2d's second axis in the light launches.  It takes more than 2^28 lanes of one launch, which within
kLightMaxVoxels only thin boxes reach (one voxel in x, so that a plane word holds one voxel), and their workspace is more
than 100 GB.

Closed forms for the cases too large for the restatements, each held against them at small sizes by the host test: cube_sky
(the sky light around a solid 64^3 cube), cube_lamps_slab (that plus block light of emitters in open air, one z-slab at a
time) and single_channel (a one-channel field from the two-channel one)."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from tests import ref_light as RL
from tests.launch_limit_cases import CAP_SOURCES as _LAUNCH_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = "voxelengine_amd/csrc/"
_shift = lambda s: 1 << int(s)

CAP_SOURCES = {  # name: (file, regex whose group 1 is the value, value from the group); each must match exactly once
    "tally_few": (_CSRC + "vxrt_light.hip", r"few = tb / \d+u < (\d+)u \? \(tb < \1u \? tb : \1u\) : tb / \d+u;", int),
    "tally_div": (_CSRC + "vxrt_light.hip", r"few = tb / (\d+)u < \d+u \? \(tb < \d+u \? tb : \d+u\) : tb / \1u;", int),
    "tally_max": (_CSRC + "vxrt_light.hip", r"k_light_tally, dim3\(\(unsigned\)\(few < (\d+)u \? few : \1u\)\)", int),
    "classify_lanes": (_CSRC + "vxrt_light.hip",
                       r"k_light_classify\(const LightArgs A\)\n\{\n    const uint32_t e = blockIdx\.x \* (\d+)u \+ threadIdx\.x;", int),
    "light_max_emitters": (_CSRC + "vxrt_light.hpp", r"kLightMaxEmitters = (\d+);", int),
    "light_max_voxels": (_CSRC + "vxrt_light.hpp", r"constexpr uint64_t kLightMaxVoxels = 1ull << (\d+);", _shift),
    "light_slab": (_CSRC + "vxrt_light.hpp", r"constexpr uint32_t kLightSlab = (\d+);", int),
    "light_halo": (_CSRC + "vxrt_light.hpp", r"kLightHalo = (\d+),", int),
    "place_launch_lanes": (_CSRC + "vxrt_place.hip", r"most = \(\(1ull << (\d+)\) \+ per_placement - 1\) / per_placement;", _shift),
    "place_blocks": (_CSRC + "vxrt_place.hip", r"return \(unsigned\)\(b > (\d+) \? \1 : ", int),
    "place_max_dim": (_CSRC + "vxrt_place.hpp", r"constexpr int32_t kPlaceMaxDim = (\d+);", int),
    "place_max_voxels": (_CSRC + "vxrt_place.hpp", r"constexpr uint64_t kPlaceMaxVoxels = 1u << (\d+);", _shift),
    "grid_2d_x": _LAUNCH_SOURCES["grid_2d_x"],
}
# kPlaceMaxVoxels bounds the rows of a piece only behind kPlaceMaxDim^2: raising it alone changes no launch
CAPS_THAT_BIND = [n for n in CAP_SOURCES if n != "place_max_voxels"]


def read_caps(root=ROOT):
    caps = {}
    for name, (path, rx, value) in CAP_SOURCES.items():
        with open(os.path.join(root, path)) as f:
            found = re.findall(rx, f.read())
        assert len(found) == 1, (name, path, rx, found)
        caps[name] = value(found[0])
    return caps


def ceil_div(a, b):
    return -(-a // b)


class Case:
    """a name, the path it targets (file: what), its shape, and reach(caps) -> [(what, value, bound)]: value > bound each"""

    def __init__(self, name, path, shape, reach):
        self.name, self.path, self.shape, self.reach = name, path, dict(shape), reach

    def __repr__(self):
        return "Case(%s)" % self.name


SKY, BLOCK = RL.SKY, RL.BLOCK
MASKS = (SKY, BLOCK, SKY | BLOCK)


# ---- the launch arithmetic of vxrt_light.hip, restated
def box_words(d0, caps):
    """light_box_words: the halo words per row that hold voxels of the box"""
    return ((caps["light_halo"] + d0 - 1) >> 5) + 1


def tally_words(dims, caps):
    """nt: the words k_light_tally visits"""
    return box_words(dims[0], caps) * dims[1] * dims[2]


def tally_groups(dims, caps):
    """(tb, the workgroups of k_light_tally)"""
    tb = ceil_div(tally_words(dims, caps), 256)
    few = min(tb, caps["tally_few"]) if tb // caps["tally_div"] < caps["tally_few"] else tb // caps["tally_div"]
    return tb, min(few, caps["tally_max"])


def tally_word_index(dims, caps):
    """int64 [x, y, z]: the index of k_light_tally's word that holds each voxel of the box"""
    x = (np.arange(dims[0], dtype=np.int64) + caps["light_halo"]) >> 5
    y = np.arange(dims[1], dtype=np.int64)
    z = np.arange(dims[2], dtype=np.int64)
    return x[:, None, None] + box_words(dims[0], caps) * (y[None, :, None] + dims[1] * z[None, None, :])


def above_first(origin, dims, caps):
    """light_above_first: the first world row above the halo, clamped to the world's floor"""
    return max(origin[1] + dims[1] + caps["light_halo"], 0)


def above_slabs(world_height, origin, dims, caps):
    return max(ceil_div(world_height - above_first(origin, dims, caps), caps["light_slab"]), 0)


def box_solid(world, origin, dims):
    """bool [x, y, z]: the solid voxels of the box (outside the world: empty)"""
    return RL.halo_solid(world, origin, dims, halo=0)


def levels_at(levels, solid, where):
    """(sky levels, block levels) that occur among the empty voxels of the box selected by the mask `where`"""
    v = levels[where & ~solid]
    return set((v >> 4).tolist()), set((v & 15).tolist())


def single_channel(want, channels):
    """the field of one channel mask from the two-channel field `want` (tests/ref_light.py's form): the other channel reads
    0 everywhere, its histogram holds every empty voxel at level 0; without the sky channel nothing is counted exposed,
    without the block channel no emitter is classified"""
    if channels == SKY | BLOCK:
        return want
    s = want["summary"]
    dark = (sum(s[2]),) + (0,) * 15
    if channels == SKY:
        return {"levels": want["levels"] & 0xF0, "summary": (s[0], s[1], s[2], dark, s[4], 0, 0, 0, 0, 0)}
    return {"levels": want["levels"] & 0x0F, "summary": (s[0], 0, dark, s[3], 0, s[5], *s[6:10])}


# ---- LIGHT_EMITTERS_65536
# A 64^3 leaky-roof world; the box is 84 wide so that two whole plane words of a row (halo x 32 .. 95) lie inside it.
EM_ORIGIN, EM_DIMS, EM_ROOF = (-10, 22, 12), (84, 20, 40), 32
EM_ROW = (8, 36, 30)          # the run of 64 one-level emitters: x = 8 .. 71 at this y, z (world x 8 .. 63 carved empty)
EM_SPECIAL = (255, 256, 257, 511, 512, 65535)
EM_COUNTS = (256, 257, 65536)
EM_SHARED_STEP, EM_SHARED_AT, EM_ROW_STEP, EM_ROW_AT = 16, 3, 1024, 7  # entries 16 k + 3 share a voxel, 1024 j + 7 are the run


@functools.lru_cache(maxsize=None)
def emitter_world():
    w = RL.leaky_roof_world(np.random.default_rng(41), shape=(64, 64, 64), roof_y=EM_ROOF)
    w[EM_ROW[0]:, EM_ROW[1], EM_ROW[2]] = False
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def emitter_list():
    """(entries int32 (65536, 4), class per entry: 0 used, 1 solid, 2 far, 3 invalid, the shared voxel, the special voxels).
    Per 256 entries: 16 on the shared voxel (levels cycling 1 .. 15), one used emitter of level 1 .. 5 on a voxel of its
    own, the rest solid, far (some one voxel outside the halo) and invalid ones (levels 0, 16, -1 and the ends of int32)
    in equal shares; EM_SPECIAL are used emitters of levels 9 .. 14 on distinct voxels; 64 entries 1024 apart are the run
    of level-1 emitters along EM_ROW.  Every used emitter but those of the run is more than its reach from the run."""
    world, rng, n, H = emitter_world(), np.random.default_rng(42), 65536, RL.HALO
    o, d = np.asarray(EM_ORIGIN, np.int64), np.asarray(EM_DIMS, np.int64)
    lo, hi = o - H, o + d + H
    e = np.zeros((n, 4), np.int64)
    cls = rng.integers(1, 4, n)
    a, b = np.maximum(lo, 0), np.minimum(hi, 64)
    solid = np.argwhere(world[a[0]:b[0], a[1]:b[1], a[2]:b[2]]) + a
    e[:, :3] = rng.integers(lo, hi, (n, 3))
    e[:, 3] = rng.integers(1, 16, n)
    k = cls == 1
    e[k, :3] = solid[rng.integers(0, len(solid), k.sum())]
    k = np.flatnonzero(cls == 2)
    axis, out = rng.integers(0, 3, len(k)), rng.choice([0, 1, 1000], len(k))
    e[k, axis] = np.where(rng.random(len(k)) < 0.5, lo[axis] - 1 - out, hi[axis] + out)
    k = cls == 3
    e[k, 3] = rng.choice([0, 16, -1, 2 ** 31 - 1, -2 ** 31], k.sum())
    # the used ones: empty voxels of the box
    x, y, z = np.meshgrid(*(np.arange(o[i], o[i] + d[i]) for i in range(3)), indexing="ij")
    free = ~box_solid(world, EM_ORIGIN, EM_DIMS)
    away = free & ((abs(y - EM_ROW[1]) > 6) | (abs(z - EM_ROW[2]) > 6))
    far_z = free & (z >= EM_ROW[2] + 17) & (x >= 0) & (x < 64)
    spots = np.stack([x[far_z], y[far_z], z[far_z]], 1)
    spots = spots[rng.permutation(len(spots))[:len(EM_SPECIAL) + 1]]
    shared, special = spots[0], spots[1:]
    own = np.stack([x[away], y[away], z[away]], 1)
    own = own[rng.permutation(len(own))[:n // 256]]
    offsets = [t for t in range(2, 255) if t % EM_SHARED_STEP != EM_SHARED_AT and t != EM_ROW_AT]
    at = 256 * np.arange(n // 256) + rng.choice(offsets, n // 256)
    e[at, :3], e[at, 3], cls[at] = own, rng.integers(1, 6, len(at)), 0
    at = EM_SHARED_STEP * np.arange(n // EM_SHARED_STEP) + EM_SHARED_AT
    e[at, :3], e[at, 3], cls[at] = shared, 1 + np.arange(len(at)) % 15, 0
    at = EM_ROW_STEP * np.arange(64) + EM_ROW_AT
    e[at, 0], e[at, 1], e[at, 2], e[at, 3], cls[at] = EM_ROW[0] + np.arange(64), EM_ROW[1], EM_ROW[2], 1, 0
    at = np.asarray(EM_SPECIAL)
    e[at, :3], e[at, 3], cls[at] = special, 9 + np.arange(len(at)), 0
    e, cls = e.astype(np.int32), cls.astype(np.int64)
    e.setflags(write=False)
    cls.setflags(write=False)
    return e, cls, tuple(int(v) for v in shared), [tuple(int(v) for v in s) for s in special]


LIGHT_EMITTERS_65536 = Case(
    "light_emitters_65536", "vxrt_light.hip: k_light_classify / k_light_scatter over 256 workgroups",
    dict(world=(64, 64, 64, 8), origin=EM_ORIGIN, dims=EM_DIMS, counts=EM_COUNTS),
    lambda c: [("entries", max(EM_COUNTS), c["light_max_emitters"] - 1),
               ("emitter workgroups", ceil_div(max(EM_COUNTS), c["classify_lanes"]), 255),
               ("entries of the shortest list of two workgroups", sorted(EM_COUNTS)[1], c["classify_lanes"]),
               ("distance of two entries on the shared voxel's word", c["classify_lanes"], EM_SHARED_STEP)])

# ---- LIGHT_TALLY_STRIDE
STRIDE_ORIGIN, STRIDE_DIMS, STRIDE_EDGE = (14, 14, 14), (100, 100, 100), 128


@functools.lru_cache(maxsize=None)
def stride_world():
    w = RL.leaky_roof_world(np.random.default_rng(43), shape=(STRIDE_EDGE,) * 3, roof_y=STRIDE_EDGE // 2)
    w[:, STRIDE_EDGE // 2 + 16:, :] = False  # open air from 16 rows above the roof: the sky reaches the noise and the roof's holes
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def stride_emitters():
    """level-15 emitters on empty voxels of the box, eight of them in its last slices (z >= 98), and weaker ones"""
    world, rng = stride_world(), np.random.default_rng(44)
    free = np.argwhere(~box_solid(world, STRIDE_ORIGIN, STRIDE_DIMS)) + np.asarray(STRIDE_ORIGIN)
    last = free[free[:, 2] >= 98]
    rows = [(*last[i], 15) for i in rng.integers(0, len(last), 8)] + [(*free[i], 15) for i in rng.integers(0, len(free), 8)]
    rows += [(*free[i], int(rng.integers(1, 15))) for i in rng.integers(0, len(free), 24)]
    return tuple(tuple(int(v) for v in r) for r in rows)


LIGHT_TALLY_STRIDE = Case(
    "light_tally_stride", "vxrt_light.hip: k_light_tally's grid-stride loop, second pass",
    dict(world=(128, 128, 128, 16), origin=STRIDE_ORIGIN, dims=STRIDE_DIMS),
    lambda c: [("tally words", tally_words(STRIDE_DIMS, c), c["tally_few"] * 256),
               ("tally words", tally_words(STRIDE_DIMS, c), tally_groups(STRIDE_DIMS, c)[1] * 256)])

# ---- the cube world of LIGHT_TALLY_CAP, LIGHT_MAX_VOXELS and the clamp of LIGHT_ABOVE_SLABS
CUBE = 64
CAP_ORIGIN, CAP_DIMS = (20, -698, -698), (1, 1460, 1460)


def cube_world():
    return np.ones((CUBE, CUBE, CUBE), bool)


def _grid(origin, dims):
    x, y, z = (np.arange(o, o + d, dtype=np.int64) for o, d in zip(origin, dims))
    return x[:, None, None], y[None, :, None], z[None, None, :]


def cube_sky(origin, dims):
    """(sky int64, solid bool, exposed bool), each [x, y, z] over the box, around the solid cube [0, 64)^3: inside it the
    voxels are solid and dark; under its footprint at y < 0 no voxel sees the sky, and the light of the nearest open column
    arrives level with the voxel, 15 less the steps to it, min(x + 1, 64 - x, z + 1, 64 - z) (a level above 0 needs at most 14
    steps: inside the halo of any box); every other voxel sees the sky"""
    x, y, z = _grid(origin, dims)
    foot = (x >= 0) & (x < CUBE) & (z >= 0) & (z < CUBE)
    solid = foot & (y >= 0) & (y < CUBE)
    steps = np.minimum(np.minimum(x + 1, CUBE - x), np.minimum(z + 1, CUBE - z))
    sky = np.where(solid, 0, np.where(foot & (y < 0), np.maximum(15 - steps, 0), 15))
    return sky, solid, np.broadcast_to(~foot | (y >= CUBE), sky.shape)


def cube_field(origin, dims):
    """cube_sky as a two-channel field without emitters, in the restatements' form"""
    sky, solid, exposed = cube_sky(origin, dims)
    return RL.pack(sky, np.zeros_like(sky), solid, exposed, (0, 0, 0, 0))


LIGHT_TALLY_CAP = Case(
    "light_tally_cap", "vxrt_light.hip: k_light_tally at its cap of workgroups",
    dict(world=(64, 64, 64, 8), origin=CAP_ORIGIN, dims=CAP_DIMS),
    lambda c: [("tb / div", tally_groups(CAP_DIMS, c)[0] // c["tally_div"], c["tally_max"]),
               ("tb / div", tally_groups(CAP_DIMS, c)[0] // c["tally_div"], c["tally_few"]),
               ("tally words", tally_words(CAP_DIMS, c), c["tally_max"] * 256)])

# ---- LIGHT_MAX_VOXELS
MAXV_ORIGIN, MAXV_DIMS, MAXV_SLAB = (-300, -200, -200), (1024, 512, 512), 32


def _cube_distance(p):
    """the largest of the three axis distances from voxel p to the cube: more than r means the cube is outside p's reach r"""
    return max(max(-v, v - (CUBE - 1), 0) for v in p)


def open_air_lamps(origin, dims, n, seed):
    """emitter entries for a box around the cube: `n` used ones on voxels of the box more than 30 voxels from the cube (the
    box's first and last voxel among them, and three on one voxel with levels 4, 13 and 9), one inside the cube, one a voxel
    outside the halo and one of level 16.  Returns (entries, counts by class)"""
    rng = np.random.default_rng(seed)
    o, d = np.asarray(origin, np.int64), np.asarray(dims, np.int64)
    rows = [(*o, 15), (*(o + d - 1), 14)]
    assert all(_cube_distance(r[:3]) > 30 for r in rows)
    while len(rows) < n - 2:
        p = tuple(int(v) for v in rng.integers(o, o + d))
        if _cube_distance(p) > 30:
            rows.append((*p, int(rng.integers(1, 16))))
    twin = rows[2][:3]
    rows[2] = (*twin, 4)
    rows += [(*twin, 13), (*twin, 9)]
    rows += [(CUBE // 2, CUBE // 2, CUBE // 2, 15), (int(o[0]) - RL.HALO - 1, int(o[1]), int(o[2]), 15), (*twin, 16)]
    return tuple(tuple(int(v) for v in r) for r in rows), (n, 1, 1, 1)


def _clip(lo, hi, a, b):
    return max(lo, a), min(hi, b)


def cube_lamps_slab(origin, dims, lamps, z0, z1):
    """the packed levels (sky << 4 | block) of the slices z0 .. z1 - 1 of the box as uint8 [z, y, x] -- the order of the
    output -- for the cube world and `lamps` (open_air_lamps): 0xF0 everywhere, the sky nibble from cube_sky over the cube's
    footprint, the block nibble max(level - L1 distance) over each used lamp's reach, which holds no solid voxel"""
    out = np.full((z1 - z0, dims[1], dims[0]), 0xF0, np.uint8)
    ax, bx = _clip(origin[0], origin[0] + dims[0], 0, CUBE)
    az, bz = _clip(origin[2] + z0, origin[2] + z1, 0, CUBE)
    if ax < bx and az < bz:
        sky, _, _ = cube_sky((ax, origin[1], az), (bx - ax, dims[1], bz - az))
        out[az - origin[2] - z0:bz - origin[2] - z0, :, ax - origin[0]:bx - origin[0]] = (sky << 4).astype(np.uint8).transpose(2, 1, 0)
    for px, py, pz, level in lamps:
        p = (px, py, pz)
        if not 1 <= level <= 15 or _cube_distance(p) <= 30:
            continue
        r = level - 1
        lo = [max(p[k] - r, origin[k] + (z0 if k == 2 else 0)) for k in range(3)]
        hi = [min(p[k] + r + 1, origin[k] + (z1 if k == 2 else dims[k])) for k in range(3)]
        if any(a >= b for a, b in zip(lo, hi)):
            continue
        x, y, z = _grid(lo, [b - a for a, b in zip(lo, hi)])
        blk = np.maximum(level - (abs(x - px) + abs(y - py) + abs(z - pz)), 0).astype(np.uint8).transpose(2, 1, 0)
        sub = out[lo[2] - origin[2] - z0:hi[2] - origin[2] - z0, lo[1] - origin[1]:hi[1] - origin[1], lo[0] - origin[0]:hi[0] - origin[0]]
        sub[...] = (sub & 0xF0) | np.maximum(sub & 0x0F, blk)
    return out


class SlabSummary:
    """the summary of a cube_lamps field, added up slab by slab"""

    def __init__(self, origin, dims, counts):
        self.origin, self.dims, self.counts = origin, dims, counts
        self.hist = np.zeros(256, np.int64)
        self.solid = 0

    def add(self, slab, z0, z1):
        self.hist += np.bincount(slab.reshape(-1), minlength=256)
        o, d = self.origin, self.dims
        side = [max(min(o[k] + (z1 if k == 2 else d[k]), CUBE) - max(o[k] + (z0 if k == 2 else 0), 0), 0) for k in range(3)]
        self.solid += side[0] * side[1] * side[2]

    def summary(self):
        """solid voxels read 0x00 and are in no histogram; a voxel is exposed unless it lies in or under the cube"""
        o, d = self.origin, self.dims
        h = self.hist.reshape(16, 16).copy()
        h[0, 0] -= self.solid
        sky, blk = h.sum(1), h.sum(0)
        foot = [max(min(o[k] + d[k], CUBE) - max(o[k], 0), 0) for k in (0, 2)]
        hidden = foot[0] * foot[1] * max(min(o[1] + d[1], CUBE) - o[1], 0)
        lv = np.arange(16)
        return (self.solid, d[0] * d[1] * d[2] - hidden, tuple(int(v) for v in sky), tuple(int(v) for v in blk),
                int((sky * lv).sum()), int((blk * lv).sum()), *self.counts)


def cube_lamps_field(origin, dims, lamps, counts, slab=MAXV_SLAB):
    """the whole field in the restatements' form (small boxes: the host test)"""
    total, parts = SlabSummary(origin, dims, counts), []
    for z0 in range(0, dims[2], slab):
        z1 = min(z0 + slab, dims[2])
        parts.append(cube_lamps_slab(origin, dims, lamps, z0, z1))
        total.add(parts[-1], z0, z1)
    return {"levels": np.concatenate(parts).transpose(2, 1, 0), "summary": total.summary()}


LIGHT_MAX_VOXELS = Case(
    "light_max_voxels", "vxrt_light.hpp: a box of kLightMaxVoxels voxels",
    dict(world=(64, 64, 64, 8), origin=MAXV_ORIGIN, dims=MAXV_DIMS),
    lambda c: [("voxels", MAXV_DIMS[0] * MAXV_DIMS[1] * MAXV_DIMS[2], c["light_max_voxels"] - 1),
               ("voxels the contract leaves", c["light_max_voxels"] + 1, MAXV_DIMS[0] * MAXV_DIMS[1] * MAXV_DIMS[2])])

# ---- LIGHT_ABOVE_SLABS
TALL = (64, 4160, 64)
ABOVE_ORIGIN, ABOVE_DIMS = (0, 4, 0), (40, 10, 40)
ABOVE_COLUMNS = ((5, 5), (15, 9), (25, 20), (33, 30))  # (x, z) of the four single voxels, in the order of above_heights
CLAMP_BOXES = (((20, -60, 20), (5, 4, 3)), ((-3, -60, 20), (5, 4, 3)))
ABOVE_SEEN = 64  # more slabs than any launch of the other tests (about 55, on the 512-high bench world)


def above_heights(caps):
    """y of the four voxels: the world's top row, mid-height, the first row above the halo, the halo's own top row"""
    first = above_first(ABOVE_ORIGIN, ABOVE_DIMS, caps)
    return (TALL[1] - 1, TALL[1] // 2, first, first - 1)


def tall_world(caps):
    w = np.zeros(TALL, bool)
    w[:, :4, :] = True
    for (x, z), y in zip(ABOVE_COLUMNS, above_heights(caps)):
        w[x, y, z] = True
    return w


LIGHT_ABOVE_SLABS = Case(
    "light_above_slabs", "vxrt_light.hip: k_light_above over hundreds of slabs, and light_above_first clamped to row 0",
    dict(world=(*TALL, 8), origin=ABOVE_ORIGIN, dims=ABOVE_DIMS, clamp=CLAMP_BOXES),
    lambda c: [("slabs", above_slabs(TALL[1], ABOVE_ORIGIN, ABOVE_DIMS, c), ABOVE_SEEN),
               ("slab of the top row's voxel", (above_heights(c)[0] - above_heights(c)[2]) // c["light_slab"], ABOVE_SEEN),
               ("slab of the mid-height voxel", (above_heights(c)[1] - above_heights(c)[2]) // c["light_slab"], ABOVE_SEEN)] +
              [("rows from the box's top down to the world's floor", -(o[1] + d[1]), c["light_halo"]) for o, d in CLAMP_BOXES])

# ---- LIGHT_UNALIGNED_OUT
UNALIGNED_OFFSETS = (1, 2, 3)
UNALIGNED_BOXES = (((20, 25, 20), (5, 4, 3)), ((3, 28, 40), (5, 3, 3)), ((-2, 27, 9), (7, 3, 2)), ((30, 29, 30), (3, 3, 3)),
                   ((10, 26, -3), (37, 5, 3)))
LIGHT_UNALIGNED_OUT = Case(
    "light_unaligned_out", "vxrt_light.hpp: light_expand_lane's byte stores (LightArgs::wide == 0)",
    dict(world=(64, 64, 64, 8), offsets=UNALIGNED_OFFSETS, boxes=UNALIGNED_BOXES),
    lambda c: [("residues mod 4 of the voxel counts", len({d[0] * d[1] * d[2] % 4 for _, d in UNALIGNED_BOXES}), 3),
               ("odd widths", sum(d[0] % 2 for _, d in UNALIGNED_BOXES), len(UNALIGNED_BOXES) - 1),
               ("address residues mod 4", len({k % 4 for k in UNALIGNED_OFFSETS} - {0}), 2)])


@functools.lru_cache(maxsize=None)
def unaligned_world():
    w = RL.leaky_roof_world(np.random.default_rng(45), shape=(64, 64, 64), roof_y=30)
    w.setflags(write=False)
    return w


def unaligned_emitters(origin, dims):
    """three emitters on the first empty voxels of the box"""
    free = np.argwhere(~box_solid(unaligned_world(), origin, dims)) + np.asarray(origin)
    return [(*(int(v) for v in free[i]), l) for i, l in ((0, 15), (len(free) // 2, 9), (len(free) - 1, 4))]


# ---- pieces
PIECE_WORLD = (256, 256, 256, 32)


@functools.lru_cache(maxsize=None)
def piece_world():
    """a floor below y = 32 and clutter to run into along x, as tests/test_gpu_place.py's big pieces meet"""
    rng = np.random.default_rng(12)
    vox = np.zeros(PIECE_WORLD[:3], bool)
    vox[:, :32, :] = True
    vox[230:, 32:200, :40] = rng.random((26, 168, 40), dtype=np.float32) < 0.02
    vox.setflags(write=False)
    return vox


@functools.lru_cache(maxsize=None)
def piece_table(edge):
    """piece 0 a sparse 1 x edge x edge sheet (about 1000 voxels) with the last row's bit set, piece 1 one voxel, piece 2 a
    33 x 2 x 2 bar"""
    rng = np.random.default_rng(edge)
    sheet = rng.random((1, edge, edge), dtype=np.float32) < min(1000.0 / (edge * edge), 0.5)
    sheet[0, edge - 1, edge - 1] = True
    return [sheet, np.ones((1, 1, 1), bool), rng.random((33, 2, 2)) < 0.5]


SHEET_EDGE, SHEET_EDGE_TWIN = 1024, 32  # piece 0 of the device cases and of the host test's twins


def place_shape(shapes):
    """place_shape: (lanes, tasks) of a table of pieces of these dims"""
    rows = max(s[1] * s[2] for s in shapes)
    lanes = 1
    while lanes < 64 and lanes < rows:
        lanes <<= 1
    return lanes, ceil_div(rows, lanes)


def table_shapes(edge):
    return [(1, edge, edge), (1, 1, 1), (33, 2, 2)]


def place_most(shapes, caps):
    """the placements of one launch of place_pieces"""
    lanes, tasks = place_shape(shapes)
    return ceil_div(caps["place_launch_lanes"], lanes * tasks)


def sheet_rows(edge, shift=0):
    """three placements of piece 0, whatever its edge: a fit into the floor (the sheet's middle rows), a drop onto the floor
    and a sweep along x into the clutter; `shift` moves them in x and changes the distances"""
    mid = edge // 2
    return [[0, 100 + shift, 16 - mid, 128 - mid, 2, 0], [0, 100 - shift, 45 + shift % 5, 128 - mid, 1, -40 - shift % 7],
            [0, 200 - shift % 20, 40, 20 - mid, 0, 60 + shift % 9]]


def _small_rows(rng, n):
    """random placements of pieces 1 and 2 in and around the world"""
    pl = np.zeros((n, 6), np.int32)
    pl[:, 0] = rng.integers(1, 3, n)
    pl[:, 1:4] = rng.integers(-8, 256, (n, 3))
    pl[:, 4] = rng.integers(0, 3, n)
    pl[:, 5] = rng.integers(-12, 13, n)
    return pl


GRID_Y_N = 300
GRID_Y_SHEETS = (0, 1, 2, 254, 255, 256, 257, 297, 298, 299)  # placements of piece 0, three kinds in turn


def grid_y_batch(edge):
    pl = _small_rows(np.random.default_rng(21), GRID_Y_N)
    for k, i in enumerate(GRID_Y_SHEETS):
        pl[i] = sheet_rows(edge, 3 * (k // 3))[k % 3]
    return pl


def cut_batch(edge, most):
    """2 * most + 7 placements for launches of `most`: in turn a one-voxel piece far above the world that travels its whole
    distance, +-(i + 20), like no other placement of the batch; a one-voxel piece dropped onto the floor from a height that
    changes with i; and a random placement of the bar.  The placements beside the cuts are drops, blocked; four are
    invalid; three name piece 0, one of them in the last, short launch.  Returns (placements, indices beside the cuts)"""
    n = 2 * most + 7
    pl = _small_rows(np.random.default_rng(22), n)
    pl[:, 0] = 2
    i = np.arange(n)
    drop = lambda k: np.stack([1 + 0 * k, (13 * k) % 200, 32 + (7 * k) % 190, (11 * k) % 256, 1 + 0 * k, -((7 * k) % 190) - 1 - k % 5], -1)
    free = i[0::3]
    pl[free] = np.stack([1 + 0 * free, free % 256, 300 + 0 * free, 5 + 0 * free, 0 * free, np.where(free % 2, -free - 20, free + 20)], -1)
    pl[i[1::3]] = drop(i[1::3])
    cuts = np.asarray([most - 1, most, 2 * most - 1, 2 * most])
    pl[cuts] = drop(cuts)
    for k, bad in zip((5, most - 2, most + 1, n - 5), ([3, 9, 40, 9, 1, -3], [1, 9, 40, 9, 3, -3], [1, 9, 40, 9, 1, 4097], [2, (1 << 30) + 1, 40, 9, 1, -3])):
        pl[k] = bad
    for k, row in zip((most // 2 + 4, most + most // 2 + 4, n - 3), sheet_rows(edge, 6)):
        pl[k] = row
    return pl, cuts


CUT_MOST_TWIN = 32  # the twin of the host test: 2 * 32 + 7 placements, as if a launch held 32


def no_shift_maps_onto_itself(rows, lo=0):
    """no shift by k != 0 rows maps rows[lo:] onto rows of the batch: a results pointer off by whole rows cannot pass"""
    rows = np.asarray(rows)
    n = len(rows)
    for k in range(1, n):
        a = rows[lo:n - k] if lo + k <= n else rows[:0]
        if len(a) and np.array_equal(a, rows[lo + k:]):
            return False
        b = rows[max(lo, k):]
        if len(b) and np.array_equal(b, rows[max(lo, k) - k:n - k]):
            return False
    return True


INIT_BASE, INIT_EXTRA = 4099, 300


def init_base():
    """4099 placements of the one-voxel piece: random ones in and around the world, every 97th invalid, and a few that are
    certainly blocked at the first step, blocked after moving, free and overlapping"""
    rng = np.random.default_rng(23)
    pl = _small_rows(rng, INIT_BASE)
    pl[:, 0] = 0
    pl[::97, 4] = 3
    pl[5::97, 5] = 5000
    pl[1], pl[2], pl[3], pl[4] = [0, 9, 32, 9, 1, -3], [0, 9, 40, 9, 1, -12], [0, 9, 40, 9, 2, 12], [0, 9, 31, 9, 0, 5]
    pl[INIT_BASE - 1] = [0, 77, 33, 5, 1, -9]
    return pl


def sheet_reference(vox, pieces, pl):
    """tests/ref_place.place: place_shift for the sheet (its clearance grid would take gigabytes), place_clearance otherwise"""
    from tests import ref_place as RP
    how = lambda v, piece, o, axis, dist: (RP.place_shift if piece.shape[1] > 64 else RP.place_clearance)(v, piece, o, axis, dist)
    return RP.place(vox, pieces, pl, how)


def _sheet_lanes():
    lanes, tasks = place_shape(table_shapes(SHEET_EDGE))
    return lanes * tasks


def _most(c):
    return place_most(table_shapes(SHEET_EDGE), c)


CUT_N = 2 * 1024 + 7


PLACE_GRID_Y = Case(
    "place_grid_y", "vxrt_place.hip: k_place_sweep / k_place_contact on grid_2d's second axis",
    dict(world=PIECE_WORLD, placements=GRID_Y_N, sheets=GRID_Y_SHEETS),
    lambda c: [("rows of piece 0", SHEET_EDGE ** 2, min(c["place_max_dim"] ** 2, c["place_max_voxels"]) - 1),
               ("workgroups", GRID_Y_N * _sheet_lanes() // 256, c["grid_2d_x"]),
               ("placements of one launch", _most(c), GRID_Y_N - 1),
               ("sheets past the first grid row", sum(i * _sheet_lanes() // 256 >= c["grid_2d_x"] for i in GRID_Y_SHEETS), 2),
               ("sheets in the first grid row", sum((i + 1) * _sheet_lanes() // 256 <= c["grid_2d_x"] for i in GRID_Y_SHEETS), 2)])
PLACE_BATCH_CUT = Case(
    "place_batch_cut", "vxrt_place.hip: place_pieces' cut into launches of at most 2^30 lanes",
    dict(world=PIECE_WORLD, placements=CUT_N),
    lambda c: [("launches", ceil_div(CUT_N, _most(c)), 2),
               ("placements of the last launch", CUT_N % _most(c), 0),
               ("placements a launch leaves the last one", _most(c),
                CUT_N % _most(c)),
               ("edge of piece 0", SHEET_EDGE, c["place_max_dim"] - 1)])
PLACE_INIT_STRIDE = Case(
    "place_init_stride", "vxrt_place.hip: k_place_init / k_place_finish grid-stride",
    dict(world=PIECE_WORLD, placements=65536 * 256 + INIT_EXTRA, base=INIT_BASE),
    lambda c: [("placements", 65536 * 256 + INIT_EXTRA, c["place_blocks"] * 256),
               ("placements of one launch", c["place_launch_lanes"], 65536 * 256 + INIT_EXTRA - 1)])

LIGHT_CASES = [LIGHT_EMITTERS_65536, LIGHT_TALLY_STRIDE, LIGHT_TALLY_CAP, LIGHT_MAX_VOXELS, LIGHT_ABOVE_SLABS, LIGHT_UNALIGNED_OUT]
PLACE_CASES = [PLACE_GRID_Y, PLACE_BATCH_CUT, PLACE_INIT_STRIDE]
LAUNCH_CASES = LIGHT_CASES + PLACE_CASES


# ---- references computed once and shared by the tests of a session (read-only)
def _frozen(field):
    field["levels"].setflags(write=False)
    return field


@functools.lru_cache(maxsize=None)
def emitter_reference(n):
    return _frozen(RL.light_field(emitter_world(), EM_ORIGIN, EM_DIMS, emitter_list()[0][:n], SKY | BLOCK))


@functools.lru_cache(maxsize=None)
def stride_reference():
    return _frozen(RL.light_field(stride_world(), STRIDE_ORIGIN, STRIDE_DIMS, stride_emitters(), SKY | BLOCK))
