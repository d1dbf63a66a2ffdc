"""Launch-limit cases of mesh voxelization and distance fields: calls of vxrt_voxelize_mesh and vxrt_distance_field whose
shapes reach the code that only the kernels have (voxelengine_amd/csrc/vxrt_voxelize.hip, vxrt_dist.hip) and the per-lane
arithmetic at its operand limits.  Shared by tests/test_launch_limits_host.py, which holds every case to the constant it
must exceed and every identity below to the restatements, and tests/test_gpu_launch_limits.py, which runs them on the device.

The constants live in voxelengine_amd/csrc; read_caps() reads them with regexes that must match exactly once:
- k_vox_groups is one workgroup of `vox_groups_threads` threads; thread i owns per = ceil(ngroups / threads) groups of
  kVoxGroup triangles, so per >= 2 takes more than threads * kVoxGroup triangles;
- k_vox_final packs 64 / wpr whole rows of wpr words into a wave (no constant: the widths are listed in ROW_WIDTHS);
- grid_2d (vxrt_region.hpp) goes to a second grid dimension past 1 << 20 workgroups;
- distance_field picks the slab of dist_sweeps by `radius <= 32u` and `radius <= 96u`, up to kDistMaxRadius; a tile is
  kDistTile voxels.

Identities used in place of a full restatement (each held against tests/ref_voxelize.py at small sizes by the host test):
the result of a voxelization does not depend on the order of the triangles, the surface field is an OR and the solid field
a parity, so k copies of a mesh give the mesh's surface and, for even k, no solid voxel; invalid, degenerate and wholly
outside triangles change no voxel and only their counters."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from tests import ref_dist as RD
from tests import ref_voxelize as RV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = "voxelengine_amd/csrc/"

CAP_SOURCES = {  # name: (file, regex whose group 1 is the value, value from the group); each must match exactly once
    "vox_groups_threads": (_CSRC + "vxrt_voxelize.hip", r"__launch_bounds__\((\d+)\) void k_vox_groups", int),
    "vox_group": (_CSRC + "vxrt_voxelize.hpp", r"constexpr uint32_t kVoxGroup = (\d+);", int),
    "vox_max_triangles": (_CSRC + "vxrt_voxelize.hpp", r"constexpr uint32_t kVoxMaxTriangles = 1u << (\d+);", lambda s: 1 << int(s)),
    "vox_max_dim": (_CSRC + "vxrt_voxelize.hpp", r"kVoxMaxDim = (\d+),", int),
    "vox_max_coord": (_CSRC + "vxrt_voxelize.hpp", r"kVoxMaxCoord = 1 << (\d+);", lambda s: 1 << int(s)),
    "grid_2d_x": (_CSRC + "vxrt_region.hpp", r"gx = blocks > \(1u << (\d+)\) \? \(1u << \1\) :", lambda s: 1 << int(s)),
    "dist_small_radius": (_CSRC + "vxrt_dist.hip", r"\n    if \(radius <= (\d+)u\)\n\s+dist_sweeps<", int),
    "dist_mid_radius": (_CSRC + "vxrt_dist.hip", r"\n    else if \(radius <= (\d+)u\)\n\s+dist_sweeps<", int),
    "dist_tile": (_CSRC + "vxrt_dist.hpp", r"constexpr uint32_t kDistTile = (\d+);", int),
    "dist_max_radius": (_CSRC + "vxrt_dist.hpp", r"constexpr uint32_t kDistMaxRadius = (\d+),", int),
}


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


# ---- voxelization: A, many groups; B, the triangle limit -----------------------------------------------------------------------
BASE_DIMS = (48, 47, 49)
MODES = (RV.SURFACE, RV.SOLID, RV.SURFACE | RV.SOLID)


@functools.lru_cache(maxsize=None)
def base_mesh():
    v, t = RV.icosphere((24.2, 23.7, 24.4), 20.3, 3)
    assert len(t) == 1280
    return v, t


@functools.lru_cache(maxsize=None)
def base_reference(modes):
    """the reference of the base mesh in one pure mode (SURFACE or SOLID), computed once and left unchanged"""
    assert modes in (RV.SURFACE, RV.SOLID)
    r = RV.voxelize(*base_mesh(), BASE_DIMS, modes)
    r["grid"].setflags(write=False)
    return r


def expected_copies(k, modes, extra=(0, 0, 0, 0)):
    """the result of k copies of the base mesh plus `extra` = (n, invalid, degenerate, outside) inert triangles, from the
    base mesh's references by arithmetic: the surface of one copy, the solid field of one copy for odd k and none for even"""
    zero = np.zeros(BASE_DIMS, bool)
    s = base_reference(RV.SURFACE)["grid"] if modes & RV.SURFACE else zero
    f = base_reference(RV.SOLID)["grid"] if (modes & RV.SOLID) and k % 2 else zero
    g = s | f
    nt, inv, deg, out = base_reference(RV.SURFACE)["summary"][3:]
    return {"grid": g, "summary": (int(g.sum()), int(s.sum()), int(f.sum()), k * nt + extra[0], k * inv + extra[1],
                                   k * deg + extra[2], k * out + extra[3])}


def copies(k):
    v, t = base_mesh()
    return v, np.ascontiguousarray(np.tile(t, (k, 1)))


def inert_triangles(n, nv, first_outside):
    """n triangles without a work item, in turn degenerate (0, 0, 0), with an index past the nv vertices, and wholly
    outside (the three vertices from `first_outside` on); returns them and (n, invalid, degenerate, outside)"""
    kinds = np.arange(n) % 3
    t = np.zeros((n, 3), np.uint32)
    t[kinds == 1] = (0, 1, nv + 5)
    t[kinds == 2] = (first_outside, first_outside + 1, first_outside + 2)
    return t, (n, int((kinds == 1).sum()), int((kinds == 0).sum()), int((kinds == 2).sum()))


def with_inert_blocks(mesh, dims, blocks):
    """`mesh` with blocks of inert triangles spliced in: blocks = [(index of the mesh's triangle the block goes before, or
    len for the end, size)], ascending.  The outside triangle lies past the region's +y face, where it has neither a
    voxel box nor a centre box.  Returns (mesh, (n, invalid, degenerate, outside), inert mask per triangle)"""
    v, t = mesh
    top = RV.UNIT * dims[1]
    v2 = np.concatenate([v, np.array([[100, top + 1, 100], [500, top + 300, 100], [100, top + 300, 600]], np.int32)])
    parts, mask, counts, at = [], [], np.zeros(4, np.int64), 0
    for pos, size in blocks:
        parts.append(t[at:pos])
        mask.append(np.zeros(pos - at, bool))
        b, c = inert_triangles(size, len(v2), len(v))
        parts.append(b)
        mask.append(np.ones(size, bool))
        counts += c
        at = pos
    parts.append(t[at:])
    mask.append(np.zeros(len(t) - at, bool))
    return (v2, np.ascontiguousarray(np.concatenate(parts))), tuple(int(c) for c in counts), np.concatenate(mask)


SHUFFLED_BLOCKS = ((0, 1280), (17000, 1500), (40001, 1280), (53 * 1280, 1380))  # each at least 3 x 256; the last at the end


def shuffled_copies(k=53, blocks=SHUFFLED_BLOCKS, seed=53):
    """k copies in a seeded random order with blocks of inert triangles: (mesh, extra counts, inert mask)"""
    v, t = copies(k)
    t = np.ascontiguousarray(t[np.random.default_rng(seed).permutation(len(t))])
    return with_inert_blocks((v, t), BASE_DIMS, blocks)


def group_shares(nt, caps):
    """(ngroups, per, owning threads) of k_vox_groups for nt triangles"""
    ngroups = ceil_div(nt, caps["vox_group"])
    per = ceil_div(ngroups, caps["vox_groups_threads"])
    return ngroups, per, ceil_div(ngroups, per)


def empty_shares(inert, caps):
    """the threads of k_vox_groups whose whole share of groups holds inert triangles only (and at least one triangle)"""
    ngroups, per, _ = group_shares(len(inert), caps)
    span = per * caps["vox_group"]
    return [i for i in range(ceil_div(len(inert), span)) if inert[i * span:(i + 1) * span].all()]


def _groups_reach(nt, per_above):
    def reach(c):
        ngroups, per, owners = group_shares(nt, c)
        return [("groups", ngroups, per_above * c["vox_groups_threads"]), ("groups per thread", per, per_above),
                ("idle slots of the last owning thread's share", owners * per - ngroups, 0),
                ("threads that own nothing", c["vox_groups_threads"] - owners, 0)]
    return reach


_SHUFFLED_NT = 53 * 1280 + sum(n for _, n in SHUFFLED_BLOCKS)
MANY_GROUPS = [
    Case("copies_53", "vxrt_voxelize.hip: k_vox_groups with two groups per thread, the last share partial",
         dict(k=53, shuffled=False), _groups_reach(53 * 1280, 1)),
    Case("copies_157", "vxrt_voxelize.hip: k_vox_groups with four groups per thread", dict(k=157, shuffled=False),
         _groups_reach(157 * 1280, 3)),
    Case("copies_52", "vxrt_voxelize.hip: k_vox_groups, an even number of copies (no solid voxel)", dict(k=52, shuffled=False),
         lambda c: _groups_reach(52 * 1280, 1)(c)[:2]),
    Case("copies_53_shuffled", "vxrt_voxelize.hip: k_vox_groups shares without an item; vxrt_voxelize.hpp: vox_find over runs of "
         "empty groups", dict(k=53, shuffled=True),
         lambda c: _groups_reach(_SHUFFLED_NT, 1)(c) + [("smallest inert block", min(n for _, n in SHUFFLED_BLOCKS), 3 * c["vox_group"] - 1)]),
]

LIMIT_STRIDE = ((1 << 24) - 1) // 1279
TRIANGLE_LIMIT = Case(
    "triangles_2_24", "vxrt_voxelize.hip: k_vox_groups with 256 groups per thread; 65536 setup workgroups",
    dict(nt=1 << 24, dims=BASE_DIMS, modes=3),
    lambda c: [("triangles", 1 << 24, c["vox_max_triangles"] - 1),
               ("groups per thread", group_shares(1 << 24, c)[1], c["vox_groups_threads"] - 1),
               ("group of the last base triangle", int(limit_positions(1 << 24)[-1]) // c["vox_group"], group_shares(1 << 24, c)[0] - 2),
               ("base triangles of the first group", int((limit_positions(1 << 24) < c["vox_group"]).sum()), 0)])


def limit_positions(nt):
    """where the base mesh's 1280 triangles go among nt: a fixed stride from 0, the last one at nt - 1"""
    pos = np.arange(1280, dtype=np.int64) * ((nt - 1) // 1279)
    pos[-1] = nt - 1
    return pos


def scattered_in_degenerates(nt):
    """nt triangles, all the degenerate (0, 0, 0) but the base mesh's at limit_positions(nt); the expected result is
    expected_copies(1, modes, (nt - 1280, 0, nt - 1280, 0))"""
    v, t = base_mesh()
    out = np.zeros((nt, 3), np.uint32)
    out[limit_positions(nt)] = t
    return v, out


# ---- voxelization: C, row widths -------------------------------------------------------------------------------------------
ROW_WIDTHS = (1, 32, 33, 513, 672, 673, 992, 993, 1024)  # words per row 1, 1, 2, 17, 21, 22, 31, 32, 32
ROW_YZ = (5, 7)                                            # 35 rows: no multiple of 2, 3, 32 or 64
ROW_MODES = (RV.SOLID, RV.SURFACE | RV.SOLID)
WIDE_DIMS = (1024, 64, 64)                                 # 4096 rows of 32 words


def row_boxes(dims, seed, n=20):
    """n closed axis-aligned boxes as one mesh: x extents random over the whole row, the first two overhanging both ends of
    it (as far as the coordinate limit allows), y and z extents random over the region and a little beyond; the boxes
    overlap, so the parity alternates along a row"""
    rng = np.random.default_rng(seed)
    hi = [RV.UNIT * d for d in dims]
    vs, ts = [], []
    for i in range(n):
        lo3, hi3 = [], []
        for k in range(3):
            a, b = sorted(int(c) for c in rng.integers(-hi[k] // 8 - 300, hi[k] + hi[k] // 8 + 300, 2))
            if k == 0 and i < 2:
                a, b = -300 - i, hi[0] + 300 + i
            lo3.append(max(a, -RV.MAX_COORD))  # a coordinate past the limit would make the triangle invalid: at 1024
            hi3.append(min(b + 1, RV.MAX_COORD))  # voxels the row ends at the limit, and a box reaches its end, no further
        v, t = RV.box_mesh(lo3, hi3)
        ts.append(t + np.uint32(8 * i))
        vs.append(v)
    return np.ascontiguousarray(np.concatenate(vs)), np.ascontiguousarray(np.concatenate(ts))


def rows_per_wave(d0):
    return 64 // ceil_div(d0, 32)


@functools.lru_cache(maxsize=None)
def row_case(d0):
    """(mesh, dims) of the row-width case of width d0, or of the 4096-row case for d0 = 'wide'"""
    dims = WIDE_DIMS if d0 == "wide" else (d0,) + ROW_YZ
    return row_boxes(dims, 1000 + dims[0] + dims[1]), dims


@functools.lru_cache(maxsize=None)
def row_reference(d0, modes):
    mesh, dims = row_case(d0)
    r = RV.voxelize(*mesh, dims, modes)
    r["grid"].setflags(write=False)
    return r


def run_words(grid):
    """per row (y, z) of a bool [x, y, z] grid: the number of different 32-voxel words in which a solid run starts, and in
    which one ends"""
    g = np.concatenate([np.zeros((1,) + grid.shape[1:], bool), grid, np.zeros((1,) + grid.shape[1:], bool)])
    starts, ends = g[1:-1] & ~g[:-2], g[1:-1] & ~g[2:]
    nw = ceil_div(grid.shape[0], 32)
    pad = nw * 32 - grid.shape[0]
    per_word = lambda m: np.concatenate([m, np.zeros((pad,) + m.shape[1:], bool)]).reshape(nw, 32, *m.shape[1:]).any(1).sum(0)
    return per_word(starts), per_word(ends)


ROW_CASES = [Case("row_width_%d" % d0, "vxrt_voxelize.hip: k_vox_final with %d rows of %d words per wave" % (rows_per_wave(d0), ceil_div(d0, 32)),
                  dict(d0=d0), lambda c, d0=d0: [("rows left to the last wave", (ROW_YZ[0] * ROW_YZ[1]) % rows_per_wave(d0), 0)])
             for d0 in ROW_WIDTHS]
ROW_CASES.append(Case("row_width_1024_wide", "vxrt_voxelize.hip: k_vox_final over 4096 rows of 32 words", dict(d0="wide"),
                      lambda c: [("workgroups of the final pass", WIDE_DIMS[1] * WIDE_DIMS[2] // 2 // 4, 1),
                                 ("words per row", ceil_div(WIDE_DIMS[0], 32), 31)]))


# ---- voxelization: D, coordinate extremes -------------------------------------------------------------------------------------
def coordinate_limit_meshes():
    """the closed box over the whole coordinate range (-2^18 .. 2^18)^3, and four triangles between extreme corners"""
    M = RV.MAX_COORD
    box = RV.box_mesh((-M, -M, -M), (M, M, M))
    v = np.array([[-M, -M, -M], [M, M, M - 1], [M, -M, M], [-M, M, -M + 3], [M - 5, M, -M], [-M, -M + 7, M]], np.int32)
    return box, (v, np.array([[0, 1, 2], [3, 4, 5], [0, 4, 5], [1, 3, 2]], np.uint32))


def coordinate_limit_dims(axis):
    dims = [3, 2, 3]
    dims[axis] = RV.MAX_DIM
    return tuple(dims)


EXTREME_SLAB = (1024, 40, 1024)  # the four triangles over many blocks and columns, mode 3
COORDINATE_CASES = [Case("coordinate_limits", "vxrt_voxelize.hpp: plane terms of 2^59 and the 64-bit floor division as the device "
                         "compiler lowers them", dict(dims=[coordinate_limit_dims(a) for a in range(3)] + [EXTREME_SLAB]),
                         lambda c: [("largest coordinate", int(np.abs(coordinate_limit_meshes()[1][0]).max()), c["vox_max_coord"] - 1),
                                    ("longest dimension", max(EXTREME_SLAB), c["vox_max_dim"] - 1)])]


# ---- distance fields ----------------------------------------------------------------------------------------------------------
DIST_MODES = (RD.TO_SOLID, RD.TO_EMPTY)
RADIUS_BOX = (130, 70, 129)      # at least two tiles per axis, no dimension a multiple of the tile
RADIUS_GROUPS = {"small": (32, 33), "mid": (96, 97), "large": (255,)}  # the radii that share a world
RADII = tuple(r for g in RADIUS_GROUPS.values() for r in g)


def dense_world(shape, solid, points):
    """the tiled-linear bit words (oracle/vxo.py, dense_from_voxels) of a world of `shape` that is all solid or all empty
    except at the distinct voxels `points`"""
    X, Y, Z = shape
    assert X % 8 == 0 and Y % 8 == 0 and Z % 8 == 0
    words = np.full(X * Y * Z // 32, 0xFFFFFFFF if solid else 0, np.uint32)
    p = np.asarray(points, np.int64).reshape(-1, 3)
    assert len(np.unique(p, axis=0)) == len(p) and (p >= 0).all() and (p < np.asarray(shape)).all()
    t, i = p >> 3, p & 7
    bit = ((((t[:, 2] * (Y // 8) + t[:, 1]) * (X // 8) + t[:, 0]) * 8 + i[:, 2]) * 8 + i[:, 1]) * 8 + i[:, 0]
    np.bitwise_xor.at(words, bit >> 5, np.uint32(1) << (bit & 31).astype(np.uint32))
    return words


def radius_anchors(R):
    """(output voxel, its target) pairs in box coordinates: the target R away along one axis alone, from a voxel of the
    box's last or first row, slice or column, so that the outermost row of a slab decides the value.  Odd radii sit 16
    voxels aside of even ones: two radii share a world.  The y and z anchors keep to the box's last columns, which are
    more than R inside the world where the box overhangs it at x < 0 (TO_EMPTY)."""
    s = 16 * (R & 1)
    bx, by, bz = (d - 1 for d in RADIUS_BOX)
    return [((bx - 2 - s, by, 20), (bx - 2 - s, by + R, 20)),    # +y: the last halo row, past the last tile
            ((bx - 3 - s, 10, bz), (bx - 3 - s, 10, bz + R)),    # +z: the last halo slice
            ((bx - 4 - s, 0, 110), (bx - 4 - s, -R, 110)),       # -y: halo row 0
            ((bx - 5 - s, 60, 0), (bx - 5 - s, 60, -R)),         # -z: halo slice 0
            ((0, 35 + s, 64), (-R, 35 + s, 64)),                 # -x
            ((bx, 35 + s, 70), (bx + R, 35 + s, 70))]            # +x


def radius_targets(group):
    """the targets of one radius group in box coordinates: the anchors' targets of each radius, one target past the last
    tile on +y and +z together, and seeded ones that no anchor voxel has within its radius + 1: anywhere in the halo for
    the small radii, at 0.75 R and more from the box for the others, so that voxels further than R from every target stay"""
    radii = RADIUS_GROUPS[group]
    Rm = max(radii)
    t = [a[1] for R in radii for a in radius_anchors(R)]
    q = int(0.7 * Rm)
    t.append((RADIUS_BOX[0] - 1, RADIUS_BOX[1] - 1 + q, RADIUS_BOX[2] - 1 + q))
    rng = np.random.default_rng(Rm)
    box = np.asarray(RADIUS_BOX)
    want = len(t) + (12 if group == "small" else 8)
    anchors = [(np.asarray(a[0]), R) for R in radii for a in radius_anchors(R)] + [(box - 1, Rm)]
    while len(t) < want:
        p = rng.integers(-Rm, box + Rm)
        away = np.maximum(np.maximum(-p, p - (box - 1)), 0)     # per axis, from the box
        if group != "small" and (away * away).sum() < (0.75 * Rm) ** 2:
            continue
        if any(((p - v) ** 2).sum() <= (R + 1) ** 2 for v, R in anchors) or tuple(int(c) for c in p) in t:
            continue
        t.append(tuple(int(c) for c in p))
    return t


def radius_case(group, mode):
    """(world shape, origin, targets in world coordinates and inside the world): TO_SOLID, solid voxels of an empty world
    and a box that overhangs the world at x < 0; TO_EMPTY, holes of an all-solid world, the box overhanging it at x < 0
    for R < 130 and, for R = 255, starting 200 voxels inside it (a box 130 wide that touched the outside would hold no
    voxel further than 255 from it), where its halo still starts outside and the outside is within R of its first columns"""
    Rm = max(RADIUS_GROUPS[group])
    shape = (640, 640, 640) if group == "large" else (384, 384, 384)
    origin = (200 if (group == "large" and mode == RD.TO_EMPTY) else -10, Rm + 5, Rm + 1)
    t = np.asarray(radius_targets(group), np.int64) + np.asarray(origin)
    t = t[((t >= 0) & (t < np.asarray(shape))).all(1)]
    return shape, origin, [tuple(int(c) for c in p) for p in t]


@functools.lru_cache(maxsize=None)
def radius_reference(group, R, mode):
    shape, origin, targets = radius_case(group, mode)
    r = RD.distance_field_points(shape, targets, origin, RADIUS_BOX, R, mode)
    r["dist2"].setflags(write=False)
    return r


def nearest_along_one_axis(group, R, mode, axis):
    """the output voxels (box coordinates) whose value is R^2 and whose every nearest target is R away along `axis` alone"""
    shape, origin, targets = radius_case(group, mode)
    d2 = radius_reference(group, R, mode)["dist2"]
    found = []
    for v in np.argwhere(d2 == R * R):
        diff = np.asarray(targets, np.int64) - (v + np.asarray(origin))
        near = diff[(diff * diff).sum(1) == R * R]
        others = [k for k in range(3) if k != axis]
        if len(near) and (np.abs(near[:, axis]) == R).all() and (near[:, others] == 0).all():
            found.append(tuple(int(c) for c in v))
    return found


def _radius_reach(R):
    def reach(c):
        out = [("tiles along axis %d" % k, ceil_div(d, c["dist_tile"]), 1) for k, d in enumerate(RADIUS_BOX)]
        out += [("voxels of the last tile along axis %d short of a tile" % k, (-d) % c["dist_tile"], 0) for k, d in enumerate(RADIUS_BOX)]
        lo = {32: 0, 33: c["dist_small_radius"], 96: c["dist_small_radius"], 97: c["dist_mid_radius"], 255: c["dist_max_radius"] - 1}[R]
        out.append(("radius", R, lo))
        hi = {32: c["dist_small_radius"], 33: c["dist_mid_radius"], 96: c["dist_mid_radius"], 97: c["dist_max_radius"],
              255: c["dist_max_radius"]}[R]
        out.append(("room below the instantiation's last radius", hi + 1, R))
        if R == 255:
            out.append(("slab rows cut on the last tile (64 + 2R against the rows left)", c["dist_tile"] + 2 * R,
                        RADIUS_BOX[1] + 2 * R - c["dist_tile"] * (ceil_div(RADIUS_BOX[1], c["dist_tile"]) - 1)))
        return out
    return reach


RADIUS_CASES = [Case("radius_%d" % R, "vxrt_dist.hip: dist_sweeps<%d> at its %s radius" %
                     (128 if R <= 32 else 256 if R <= 96 else 574, "last" if R in (32, 96, 255) else "first"),
                     dict(R=R, group=g), _radius_reach(R)) for g, radii in RADIUS_GROUPS.items() for R in radii]


def radius_sides(caps):
    """per threshold of distance_field, the radii of RADII at it and one past it"""
    return {t: ([R for R in RADII if R == t], [R for R in RADII if R == t + 1])
            for t in (caps["dist_small_radius"], caps["dist_mid_radius"])}


LONG_Z = dict(dims=(1, 1, 1 << 21), radius=1, world=(64, 64, 64), density=0.05, seed=21, origin=(30, 30, 40 - (1 << 21)))
SECOND_GRID = Case(
    "ysweep_2_21_slices", "vxrt_dist.hip: k_dist_ysweep past the first grid dimension (blockIdx.y > 0)", LONG_Z,
    lambda c: [("y-sweep workgroups", LONG_Z["dims"][2] + 2 * LONG_Z["radius"], c["grid_2d_x"]),
               ("first halo slice of the world", -(LONG_Z["origin"][2] - LONG_Z["radius"]), c["grid_2d_x"])])


def long_z_world():
    return np.random.default_rng(LONG_Z["seed"]).random(LONG_Z["world"]) < LONG_Z["density"]


LONG_BOXES = (((-4900, 62, 40), (5000, 3, 2)), ((50, -4929, 60), (2, 5000, 3)))  # reach the surface of a 128^3 terrain from far outside
LONG_RADIUS = 7
LONG_CASES = [Case("long_box_axis_%d" % k, "vxrt_dist.hip: a box of 5000 voxels along axis %d" % k, dict(origin=o, dims=d),
                   lambda c, d=d: [("longest axis", max(d), 1024), ("tiles along it", ceil_div(max(d), c["dist_tile"]), 16)])
              for k, (o, d) in enumerate(LONG_BOXES)]

LAUNCH_CASES = MANY_GROUPS + [TRIANGLE_LIMIT] + ROW_CASES + COORDINATE_CASES + RADIUS_CASES + [SECOND_GRID] + LONG_CASES
