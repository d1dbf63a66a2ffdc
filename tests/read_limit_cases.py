"""Read limit cases: calls of vxrt_read_region, vxrt_extract_surface, vxrt_frame_guides and vxrt_denoise_frame whose shapes
reach the code that only runs past a launch cap or at the largest values the contract allows.  Shared by
tests/test_read_limits_host.py, which holds every case to the cap it must exceed, the launch arithmetic below to the figures
worked out by hand, and every identity below to the restatements (oracle/ref_region.py, tests/ref_surface.py,
tests/ref_denoise.py) at small sizes, and tests/test_gpu_read_limits.py, which runs the cases on the device.

The caps live in voxelengine_amd/csrc; read_caps() reads them with regexes that must match exactly once:
- read_region (vxrt_region.hip) gives a row of wpr words L = min(2^ceil(log2 wpr), 2^6) lanes, so that a wave holds 64 / L
  rows or one of nxc = ceil(wpr / 64) chunks of a row; a workgroup steps through 4 * zsteps slices, zsteps starting at 8
  and halved while the launch would have fewer than 2048 workgroups; grid_2d (vxrt_region.hpp) takes the launch to a
  second grid axis past 2^20 workgroups, and the workgroups it adds to fill the last grid row must write nothing;
- the surface scan (vxrt_surface.hip) gives each of the 256 threads of k_surf_groups a share of ceil(ngroups / 256) groups
  of kSurfGroup rows; kSurfMaxDim and kSurfMaxVoxels bound the box;
- the denoiser (vxrt_denoise.hpp) takes frames of at most kDnMaxSide a side and kDnMaxPixels pixels through at most
  kDnMaxIterations iterations, in tiles of kDnTileW x 4 (DIRECT) or kDnTileW x 4 kDnStagedRows (STAGED, steps up to
  kDnMaxStagedStep) pixels.
Every case names the caps it must exceed.

Not reachable, so not covered:
- grid_2d's second axis in the surface launches: within kSurfMaxVoxels = 2^28 and kSurfMaxDim = 1024 two sides of 1024
  leave 256 for the third, so a box has at most 2 * 256 * 1024 + 4 * 1024 * 1024 = 4 718 592 rows (case 5), little more
  than 2^22, which is 18 432 workgroups of 256 rows (about 2^14), and at most 2 * 1024 * 1024 lanes of the x directions,
  2^13 workgroups: both far below 2^20;
- grid_2d's second axis in the LOD reduce: a wave task covers 64 lanes, a cell row takes at least one lane, and a box of
  2^32 source voxels has the most cell rows when it is one cell wide: 2^32 / f^3 of them, so 2^23, 2^20 and 2^17 tasks at
  shifts 1, 2 and 3; a wave takes 16, 4 and 1 tasks there and a workgroup holds four waves: at most 2^17 workgroups;
- the kSurfMaxIndexed clamp of the capacity (2^30 quads): a box of 2^28 voxels has at most 6 * 2^27 < 2^30 quads (the
  checkerboard of case 6 reaches that number).

The frames of case 8 are the issue's: 8190 x 8194 is 4 pixels short of kDnMaxPixels; 65535 x 1023 and its transpose are
the largest frames with a side of kDnMaxSide whose sides the tiles 255 x 93 / 93 x 255 divide (65535 = 255 * 257,
1023 = 93 * 11): one row and 1024 pixels short of the largest frame of that side.

Identities for the cases too large for the restatements, each held against them at small sizes by the host test:
translated (a surface of a world strictly inside its box from the surface of the world's own box), checker_* (the
surface of the 3-D parity checkerboard) and tiled_* (a frame made of copies of a small frame whose keys differ from tile
to tile denoises to copies of the small frame's result)."""
from __future__ import annotations

import functools
import os
import re
from types import SimpleNamespace

import numpy as np

from tests import ref_denoise as RD
from tests import ref_surface as RS
from tests.launch_limit_cases import CAP_SOURCES as _LAUNCH_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = "voxelengine_amd/csrc/"
_shift = lambda s: 1 << int(s)
INT32_MAX = 2 ** 31 - 1

CAP_SOURCES = {  # name: (file, regex whose group 1 is the value, value from the group); each must match exactly once
    "grid_2d_x": _LAUNCH_SOURCES["grid_2d_x"],
    "zsteps_start": (_CSRC + "vxrt_region.hip", r"\n    A\.zsteps = (\d+);", int),
    "zsteps_blocks": (_CSRC + "vxrt_region.hip", r"\(4u \* A\.zsteps\)\) < (\d+)u\)\n        A\.zsteps >>= 1;", int),
    "lgL_max": (_CSRC + "vxrt_region.hip", r"while \(\(1u << A\.lgL\) < A\.wpr && A\.lgL < (\d+)\)", int),
    "surf_group": (_CSRC + "vxrt_surface.hpp", r"constexpr uint32_t kSurfGroup = (\d+);", int),
    "surf_max_dim": (_CSRC + "vxrt_surface.hpp", r"constexpr int32_t kSurfMaxDim = (\d+);", int),
    "surf_max_voxels": (_CSRC + "vxrt_surface.hpp", r"constexpr uint64_t kSurfMaxVoxels = 1ull << (\d+);", _shift),
    "surf_share": (_CSRC + "vxrt_surface.hip", r"per = \(A\.ngroups \+ 255u\) / (\d+)u, a = threadIdx\.x \* per < A\.ngroups", int),
    "dn_max_side": (_CSRC + "vxrt_denoise.hpp", r"constexpr uint32_t kDnMaxSide = (\d+)u;", int),
    "dn_max_pixels": (_CSRC + "vxrt_denoise.hpp", r"constexpr uint64_t kDnMaxPixels = 1ull << (\d+);", _shift),
    "dn_max_iterations": (_CSRC + "vxrt_denoise.hpp", r"constexpr int32_t kDnMaxIterations = (\d+);", int),
    "dn_tile_w": (_CSRC + "vxrt_denoise.hpp", r"constexpr uint32_t kDnTileW = (\d+)u, kDnStagedRows = \d+u;", int),
    "dn_staged_rows": (_CSRC + "vxrt_denoise.hpp", r"constexpr uint32_t kDnTileW = \d+u, kDnStagedRows = (\d+)u;", int),
    "dn_max_staged_step": (_CSRC + "vxrt_denoise.hpp", r"constexpr uint32_t kDnMaxStagedStep = (\d+)u;", int),
}
CAPS_THAT_BIND = list(CAP_SOURCES)


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


# ---- the launch arithmetic of read_region (vxrt_region.hip), restated
def read_launch(dims, caps):
    """wpr, pad_mask, lgL, nxc, rpw (rows per wave), nyg, zsteps, blocks and the grid (gx, gy) of a read of `dims`"""
    d0, d1, d2 = (int(v) for v in dims)
    wpr = ceil_div(d0, 32)
    lgL = 0
    while (1 << lgL) < wpr and lgL < caps["lgL_max"]:
        lgL += 1
    nxc = ceil_div(wpr, 64)
    rpw = max(64 >> lgL, 1)
    nyg = ceil_div(d1, rpw)
    xy = nxc * nyg
    zsteps = caps["zsteps_start"]
    while zsteps > 1 and xy * ceil_div(d2, 4 * zsteps) < caps["zsteps_blocks"]:
        zsteps >>= 1
    blocks = xy * ceil_div(d2, 4 * zsteps)
    gx = min(blocks, caps["grid_2d_x"])
    return SimpleNamespace(wpr=wpr, pad_mask=(1 << (d0 & 31)) - 1 if d0 & 31 else 0xFFFFFFFF, lgL=lgL, L=1 << lgL, nxc=nxc, rpw=rpw,
                           nyg=nyg, zsteps=zsteps, blocks=blocks, gx=gx, gy=ceil_div(blocks, gx), surplus=gx * ceil_div(blocks, gx) - blocks)


def read_stores(dims, caps):
    """k_read_region's mapping of workgroups and lanes to words, restated: (the index of every word the launch stores, in no
    order, surplus workgroups included; (xw, yl, zl) of each)"""
    d0, d1, d2 = (int(v) for v in dims)
    A = read_launch(dims, caps)
    b = np.arange(A.gx * A.gy, dtype=np.int64)[:, None, None]
    t = np.arange(256, dtype=np.int64)[None, :, None]
    i = np.arange(A.zsteps, dtype=np.int64)[None, None, :]
    xc, rest = b % A.nxc, b // A.nxc
    yg, zg = rest % A.nyg, rest // A.nyg
    lane, wave = t & 63, t >> 6
    xw = xc * 64 + (lane & (A.L - 1))
    yl = yg * (64 >> A.lgL) + (lane >> A.lgL)
    zl = zg * (4 * A.zsteps) + wave + 4 * i
    live = np.broadcast_to((xw < A.wpr) & (yl < d1) & (zl < d2), (b.shape[0], 256, A.zsteps))
    idx = np.broadcast_to((yl + d1 * zl) * A.wpr + xw, live.shape)[live]
    at = tuple(np.broadcast_to(v, live.shape)[live] for v in (xw, yl, zl))
    return idx, at


def region_words(dims):
    return ceil_div(int(dims[0]), 32) * int(dims[1]) * int(dims[2])


@functools.lru_cache(maxsize=None)
def small_world():
    """the 64^3 world of cases 1 to 3 (factor 8)"""
    w = np.random.default_rng(51).random((64, 64, 64)) < 0.4
    w.setflags(write=False)
    return w


# ---- 1. GRID_Y_ALONG_Z: one voxel wide, 2^26 + 160 slices, the world's column inside
ALONG_Z_ORIGIN, ALONG_Z_DIMS = (37, 11, -100), (1, 1, (1 << 26) + 160)


def along_z_nonzero(world):
    """the indices of the words that read 1 (every other word reads 0)"""
    x, y, z = ALONG_Z_ORIGIN
    return np.flatnonzero(world[x, y, :]) - z


GRID_Y_ALONG_Z = Case(
    "grid_y_along_z", "vxrt_region.hip: k_read_region on grid_2d's second axis, zg over 2^21 workgroups, surplus workgroups",
    dict(world=(64, 64, 64, 8), origin=ALONG_Z_ORIGIN, dims=ALONG_Z_DIMS),
    lambda c: [("workgroups", read_launch(ALONG_Z_DIMS, c).blocks, 2 * c["grid_2d_x"]),
               ("surplus workgroups", read_launch(ALONG_Z_DIMS, c).surplus, 0),
               ("slices of a workgroup", 4 * read_launch(ALONG_Z_DIMS, c).zsteps, 4 * c["zsteps_start"] - 1),
               ("slices before the world", -ALONG_Z_ORIGIN[2], 4 * c["zsteps_start"])])

# ---- 2. GRID_Y_ALONG_ROWS: two rows of 2^26 words that end three voxels past the world's far face
ALONG_ROWS_DIMS = (INT32_MAX, 2, 1)
ALONG_ROWS_ORIGIN = (64 + 3 - INT32_MAX, 10, 20)
ALONG_ROWS_TAIL = 4  # the last words of a row: the world's 64 voxels lie in the last three


def along_rows_tail(world):
    """uint32 [2, ALONG_ROWS_TAIL]: the last words of the two rows (every word before them reads 0) -- a read whose origin is
    moved up by whole words returns the words of the row from there on (the region layout of include/vxrt.h)"""
    from oracle import ref_region
    skip = 32 * (ceil_div(ALONG_ROWS_DIMS[0], 32) - ALONG_ROWS_TAIL)
    o = (ALONG_ROWS_ORIGIN[0] + skip,) + ALONG_ROWS_ORIGIN[1:]
    d = (ALONG_ROWS_DIMS[0] - skip,) + ALONG_ROWS_DIMS[1:]
    assert o[0] < 0 and o[0] + d[0] == ALONG_ROWS_ORIGIN[0] + ALONG_ROWS_DIMS[0]
    return pack_region(ref_region.read_region(world, o, d)).reshape(2, ALONG_ROWS_TAIL)


def pack_region(vox):
    """bool [x, y, z] -> region words, padding bits 0 (the layout of include/vxrt.h, written out here)"""
    X, Y, Z = vox.shape
    rows = np.zeros((Z, Y, ceil_div(X, 32) * 32), bool)
    rows[:, :, :X] = vox.transpose(2, 1, 0)
    return np.packbits(rows, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


GRID_Y_ALONG_ROWS = Case(
    "grid_y_along_rows", "vxrt_region.hip: k_read_region on grid_2d's second axis, xc over 2^20 chunks, the 64-bit row start",
    dict(world=(64, 64, 64, 8), origin=ALONG_ROWS_ORIGIN, dims=ALONG_ROWS_DIMS),
    lambda c: [("workgroups", read_launch(ALONG_ROWS_DIMS, c).blocks, c["grid_2d_x"]),
               ("chunks of a row", read_launch(ALONG_ROWS_DIMS, c).nxc, c["grid_2d_x"] - 1),
               ("words of a row", read_launch(ALONG_ROWS_DIMS, c).wpr, (1 << 26) - 1),
               ("lanes of a row", 64, (1 << c["lgL_max"]) - 1),
               ("voxels before the world", -ALONG_ROWS_ORIGIN[0], INT32_MAX - 128),
               ("end of the box", ALONG_ROWS_ORIGIN[0] + ALONG_ROWS_DIMS[0], 64)])

# ---- 3. ZSTEPS_LADDER: the four values of zsteps
LADDER_BOXES = (((-5, 50, -9), (50, 37, 23)), ((45, -2017, -100), (33, 2049, 250)), ((-3, -2000, -301), (32, 4096, 500)),
                ((31, -900, -777), (65, 1030, 1001)))


def ladder_zsteps(caps):
    return [read_launch(d, caps).zsteps for _, d in LADDER_BOXES]


def _overhangs(o, d, world):
    return any(a < 0 or a + n > w for a, n, w in zip(o, d, world))


ZSTEPS_LADDER = Case(
    "zsteps_ladder", "vxrt_region.hip: read_region's zsteps of 1, 2, 4 and 8",
    dict(world=(64, 64, 64, 8), boxes=LADDER_BOXES),
    lambda c: [("distinct zsteps", len(set(ladder_zsteps(c))), 3),
               ("largest zsteps", max(ladder_zsteps(c)), c["zsteps_start"] - 1),
               ("smallest zsteps below 2", 2, min(ladder_zsteps(c))),
               ("workgroups of the largest", read_launch(LADDER_BOXES[3][1], c).blocks, c["zsteps_blocks"] - 1),
               ("slices cut short", sum(d[2] % (4 * z) != 0 for (_, d), z in zip(LADDER_BOXES, ladder_zsteps(c))), 3),
               ("boxes over a face, unaligned", sum(_overhangs(o, d, (64, 64, 64)) and o[0] % 32 != 0 for o, d in LADDER_BOXES), 3)])

# ---- 4. ROW_MAPPINGS: L = 8, 16, 32, 64 and one, two and three chunks to a row, on the wide world of the region tests
WIDE_WORLD = (8192, 64, 64, 8)
MAPPING_BOXES = (((-37, -3, 60), (5 * 32 - 7, 13, 9)), ((8192 - 200, 59, -2), (10 * 32 - 13, 7, 11)), ((-100, 61, 61), (22 * 32 - 1, 5, 7)),
                 ((8192 - 1000, -5, -1), (47 * 32 - 19, 6, 5)), ((-33, 30, 62), (64 * 32 - 31, 3, 6)),
                 ((8192 - 1029, -2, 58), (65 * 32 - 30, 4, 5)), ((8192 - 3001, 62, -3), (130 * 32 - 5, 3, 7)))
MAPPING_WPR = (5, 10, 22, 47, 64, 65, 130)
MAPPING_HOST = (1, 6)  # the boxes that also run through vxrt_read_region_host


@functools.lru_cache(maxsize=None)
def wide_world():
    w = np.random.default_rng(52).random(WIDE_WORLD[:3]) < 0.4
    w.setflags(write=False)
    return w


def _mappings(c):
    return [read_launch(d, c) for _, d in MAPPING_BOXES]


ROW_MAPPINGS = Case(
    "row_mappings", "vxrt_region.hip: k_read_region's lanes per row and chunks per row, ragged last words",
    dict(world=WIDE_WORLD, boxes=MAPPING_BOXES),
    lambda c: [("distinct lanes per row", len({m.L for m in _mappings(c)}), 3),
               ("widest row in lanes", max(m.wpr for m in _mappings(c)), 2 << c["lgL_max"]),
               ("lanes per row at the cap", sum(m.L == 1 << c["lgL_max"] for m in _mappings(c)), 3),
               ("distinct chunks per row", len({m.nxc for m in _mappings(c)}), 2),
               ("ragged last words", sum(d[0] % 32 != 0 for _, d in MAPPING_BOXES), len(MAPPING_BOXES) - 1),
               ("rows cut short in a wave", sum(d[1] % m.rpw != 0 for (_, d), m in zip(MAPPING_BOXES, _mappings(c)) if m.rpw > 1), 2),
               ("boxes over a face", sum(_overhangs(o, d, WIDE_WORLD[:3]) for o, d in MAPPING_BOXES), len(MAPPING_BOXES) - 1)])

# ---- the surface launches (vxrt_surface.hpp: surf_layout), restated
def surf_rows(dims):
    return 2 * dims[0] * dims[2] + 4 * dims[1] * dims[2]


def surf_share(dims, caps):
    """(groups of the scan, the groups one thread of k_surf_groups owns)"""
    groups = ceil_div(surf_rows(dims), caps["surf_group"])
    return groups, ceil_div(groups, caps["surf_share"])


def translated(surface, offset):
    """the Surface of a world in a box, from that of the same world in a box whose origin is `offset` voxels further up:
    every position and vertex moves by the offset, the order stays (the rows' order d, s, v is monotone under translation)"""
    ox, oy, oz = (int(v) for v in offset)
    assert min(ox, oy, oz) >= 0
    quads = surface.quads.copy()
    quads[:, 0] += np.uint32(ox | oy << 10 | oz << 20)
    d, x, y, z, w, h = RS.decode(surface.quads)
    assert len(quads) == 0 or (int((x + ox).max()) < 1024 and int((y + oy).max()) < 1024 and int((z + oz).max()) < 1024)
    return RS.Surface(quads, surface.vertices + 256 * np.asarray([ox, oy, oz], np.int32), surface.triangles, surface.summary)


# ---- 5. SCAN_SHARE
SHARE_DIMS, SHARE_EDGE = (256, 1024, 1024), 64
SHARE_ORIGINS = (tuple(SHARE_EDGE + 1 - d for d in SHARE_DIMS), (-1, -1, -1))  # the world in the far and in the near corner
SHARE_SEEN = 2  # the share of tests/test_gpu_surface.py (92 352 rows)


@functools.lru_cache(maxsize=None)
def share_world():
    w = np.random.default_rng(53).random((SHARE_EDGE,) * 3) < 0.5
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def share_reference():
    """the surface of the world's own box grown by one voxel, where CAP equals OPEN"""
    return RS.extract(share_world(), (-1, -1, -1), (SHARE_EDGE + 2,) * 3, RS.OPEN)


def share_offset(origin):
    return tuple(-1 - o for o in origin)


SCAN_SHARE = Case(
    "scan_share", "vxrt_surface.hip: k_surf_groups with a share of 72 groups a thread, the largest box",
    dict(world=(64, 64, 64, 8), origins=SHARE_ORIGINS, dims=SHARE_DIMS),
    lambda c: [("groups a thread", surf_share(SHARE_DIMS, c)[1], 71),
               ("groups a thread", surf_share(SHARE_DIMS, c)[1], SHARE_SEEN),
               ("longest side", max(SHARE_DIMS), c["surf_max_dim"] - 1),
               ("voxels", SHARE_DIMS[0] * SHARE_DIMS[1] * SHARE_DIMS[2], c["surf_max_voxels"] - 1),
               ("rows", surf_rows(SHARE_DIMS), 2 * c["surf_max_voxels"] // c["surf_max_dim"] + 4 * c["surf_max_dim"] ** 2 - 1)])

# ---- 6. CHECKERBOARD_COUNTS
CHECKER_WORLD = (1024, 1024, 256, 32)
CHECKER_PARITY = 1          # voxel (x, y, z) is solid when (x + y + z) & 1 == CHECKER_PARITY
CHECKER_CAPACITIES = (1, 4095, 4096)
CHECKER_THIN = (1, 1024, 8)


def checker(dims, parity=CHECKER_PARITY):
    x, y, z = np.ogrid[:dims[0], :dims[1], :dims[2]]
    return ((x + y + z) & 1) == parity


def checker_stamp_rows(dims, parity=CHECKER_PARITY):
    """uint32 [z, y]: the word that every word of row (y, z) of the checkerboard's region words equals (dims[0] % 32 == 0)"""
    assert dims[0] % 32 == 0
    y, z = np.ogrid[:dims[1], :dims[2]]
    return np.where(((y + z) & 1) == parity, np.uint32(0x55555555), np.uint32(0xAAAAAAAA)).T


def checker_summary(dims):
    """the summary of the checkerboard's own box in either mode, capacity 0: every solid voxel shows six faces, no two faces
    of a direction touch, so every face is a quad"""
    n = dims[0] * dims[1] * dims[2]
    assert n % 2 == 0
    return (n // 2, 3 * n, 3 * n, 0, (n // 2,) * 6, (n // 2,) * 6)


CHECKERBOARD_COUNTS = Case(
    "checkerboard_counts", "vxrt_surface.hip: the summary's counters at 6 * 2^27 quads",
    dict(world=CHECKER_WORLD, capacities=CHECKER_CAPACITIES),
    lambda c: [("voxels", CHECKER_WORLD[0] * CHECKER_WORLD[1] * CHECKER_WORLD[2], c["surf_max_voxels"] - 1),
               ("quads", checker_summary(CHECKER_WORLD[:3])[2], 6 * (c["surf_max_voxels"] // 2) - 1),
               ("longest side", max(CHECKER_WORLD[:3]), c["surf_max_dim"] - 1),
               ("records of the thin box in direction 0", CHECKER_THIN[1] * CHECKER_THIN[2] // 2, max(CHECKER_CAPACITIES) - 1)])

# ---- the denoiser's frames
DN_ITERATIONS, DN_SCALES = (1, 3, 6), (0.0, 0.75)
THIN_FRAMES = ((65535, 5), (5, 65535))          # (W, H)
LIMIT_FRAMES = (((8190, 8194), (130, 241)), ((65535, 1023), (255, 93)), ((1023, 65535), (93, 255)))  # (frame, tile), each (W, H)
LIMIT_ITERATIONS = (1, 6)
LIMIT_ALIASED = 1  # the frame of LIMIT_FRAMES whose output is its input


def dn_grid(W, H, staged, caps):
    th = 4 * (caps["dn_staged_rows"] if staged else 1)
    return ceil_div(W, caps["dn_tile_w"]), ceil_div(H, th)


THIN_FRAMES_CASE = Case(
    "thin_frames", "vxrt_denoise.hip: frames of kDnMaxSide pixels a side",
    dict(frames=THIN_FRAMES, iterations=DN_ITERATIONS, scales=DN_SCALES),
    lambda c: [("side", max(f), c["dn_max_side"] - 1) for f in THIN_FRAMES] +
              [("iterations", max(DN_ITERATIONS), c["dn_max_iterations"] - 1),
               ("largest step", 1 << (max(DN_ITERATIONS) - 1), c["dn_max_staged_step"]),
               ("staged steps", c["dn_max_staged_step"], 1 << (min(DN_ITERATIONS) - 1)),
               ("short side below a staged tile", 4 * c["dn_staged_rows"], min(THIN_FRAMES[0])),
               ("short side below a tile's width", c["dn_tile_w"], min(THIN_FRAMES[1])),
               ("workgroups along x", dn_grid(*THIN_FRAMES[0], True, c)[0], 1023),
               ("workgroups along y", dn_grid(*THIN_FRAMES[1], False, c)[1], 16383)])


def tile_ids(tiles_x, tiles_y):
    """int64 [tiles_y, tiles_x]: 1 .."""
    return 1 + np.arange(tiles_y, dtype=np.int64)[:, None] * tiles_x + np.arange(tiles_x, dtype=np.int64)[None, :]


def tiled_keys_row(keys, tiles_x, tiles_y, row):
    """the keys of row `row` of the tiles_y x tiles_x copies of a frame, every non-zero key XORed with tile_id << 8"""
    ids = tile_ids(tiles_x, tiles_y)
    assert ids.max() < 1 << 18
    big = np.tile(keys, (1, tiles_x))
    shift = np.repeat(ids[row] << 8, keys.shape[1])[None, :].astype(np.uint32)
    return np.where(big != 0, big ^ shift, 0).astype(np.uint32)


def tiled_keys(keys, tiles_x, tiles_y):
    return np.concatenate([tiled_keys_row(keys, tiles_x, tiles_y, r) for r in range(tiles_y)])


def tiles_share_no_key(keys, tiles_x, tiles_y):
    values = np.unique(keys[keys != 0]).astype(np.int64)
    every = values[:, None] ^ (tile_ids(tiles_x, tiles_y).reshape(-1) << 8)[None, :]
    return len(np.unique(every)) == every.size and 0 not in every


def tiled_frame(color, tiles_x, tiles_y):
    return np.tile(color, (tiles_y, tiles_x, 1))


def _tiles(frame, tile):
    return frame[0] // tile[0], frame[1] // tile[1]


PIXEL_LIMIT = Case(
    "pixel_limit", "vxrt_denoise.hip: frames of nearly kDnMaxPixels pixels",
    dict(frames=LIMIT_FRAMES, iterations=LIMIT_ITERATIONS, scales=DN_SCALES),
    lambda c: [("pixels", f[0] * f[1], c["dn_max_pixels"] - 2 * 65536) for f, _ in LIMIT_FRAMES] +
              [("pixels", max(f[0] * f[1] for f, _ in LIMIT_FRAMES), c["dn_max_pixels"] - 1024),
               ("side", max(f[0] for f, _ in LIMIT_FRAMES), c["dn_max_side"] - 1),
               ("iterations", max(LIMIT_ITERATIONS), c["dn_max_iterations"] - 1),
               ("narrowest tile in tiles' widths", min(t[0] for _, t in LIMIT_FRAMES), c["dn_tile_w"]),
               ("lowest tile in staged rows", min(t[1] for _, t in LIMIT_FRAMES), 4 * c["dn_staged_rows"]),
               ("tiles no multiple of a workgroup's", sum(t[0] % c["dn_tile_w"] != 0 and t[1] % (4 * c["dn_staged_rows"]) != 0 and t[0] % 16
                                                          != 0 and t[1] % 16 != 0 for _, t in LIMIT_FRAMES), len(LIMIT_FRAMES) - 1),
               ("frames the tiles divide", sum(f[0] % t[0] == 0 and f[1] % t[1] == 0 for f, t in LIMIT_FRAMES), len(LIMIT_FRAMES) - 1)])

# ---- 9. SPECIAL_VALUES
SPECIAL_FRAME = (130, 70)
SPECIAL_SCALES = (1e-45, 1.17549435e-38, 1e38, float("inf"))
SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0, 1e-40, -1e-44)


def special_frame():
    """the (130, 70) frame of tests/ref_denoise.py with NaN, infinities, -0.0 and denormals sprinkled over it: (colours, keys,
    the mask of the sprinkled pixels)"""
    W, H = SPECIAL_FRAME
    c, keys = RD.random_frame(W, H)
    rng = np.random.default_rng(54)
    pick = rng.random((H, W))
    c = c.copy()
    mask = np.zeros((H, W), bool)
    for i, v in enumerate(SPECIALS):
        at = (pick >= 0.02 * i) & (pick < 0.02 * (i + 1))
        ch = rng.integers(0, 3, (H, W))
        for k in range(3):
            c[at & ((ch == k) | (rng.random((H, W)) < 0.2)), k] = np.float32(v)
        mask |= at
    return c, keys, mask


SPECIAL_VALUES = Case(
    "special_values", "vxrt_denoise.hpp: dn_filter and dn_bgra8 on NaN, infinite, negative-zero and denormal operands",
    dict(frame=SPECIAL_FRAME, scales=SPECIAL_SCALES),
    lambda c: [("kinds of special colours under filtered keys", sum(bool((_special_is(v) & (special_frame()[1] != 0)).any()) for v in SPECIALS), len(SPECIALS) - 1),
               ("kinds of special colours under miss keys", sum(bool((_special_is(v) & (special_frame()[1] == 0)).any()) for v in SPECIALS), len(SPECIALS) - 1),
               ("denormal scales", sum(0 < np.float32(k) < np.finfo(np.float32).tiny for k in SPECIAL_SCALES), 0),
               ("infinite scales", sum(np.isinf(np.float32(k)) for k in SPECIAL_SCALES), 0),
               ("iterations", max(DN_ITERATIONS), c["dn_max_iterations"] - 1)])


def _special_is(v):
    c = special_frame()[0]
    v = np.float32(v)
    same = np.isnan(c) if np.isnan(v) else (c.view(np.uint32) == v.view(np.uint32))
    return same.any(-1)


# ---- 10. GUIDE_KEYS_LARGE_WORLD
GUIDE_WORLD = (8192, 512, 8192, 32)
GUIDE_FRAMES = ((160, 96),) + THIN_FRAMES
GUIDE_HITS = (-1, -7, 0, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 35) - 1, 1 << 35, (1 << 63) - 1, 12345678901, (1 << 34) + 8191)


def guide_hits(W, H, seed=0):
    """int64 [H, W]: random indices over the world and a little beyond it, misses, and GUIDE_HITS at the frame's first pixels,
    at its last ones and scattered"""
    rng = np.random.default_rng(55 + seed)
    n = W * H
    X, Y, Z = GUIDE_WORLD[:3]
    hit = rng.integers(0, X * Y * Z + (1 << 28), n, dtype=np.int64)
    hit[rng.random(n) < 0.1] = -1
    special = np.asarray(GUIDE_HITS, np.int64)
    hit[:len(special)] = special
    hit[n - len(special):] = special[::-1]
    at = rng.integers(len(special), n - len(special), 16 * len(special))
    hit[at] = np.tile(special, 16)
    return hit.reshape(H, W)


GUIDE_KEYS_LARGE_WORLD = Case(
    "guide_keys_large_world", "vxrt_denoise.hpp: guide_key's 64-bit division on hit indices of 2^32 and more",
    dict(world=GUIDE_WORLD, frames=GUIDE_FRAMES),
    lambda c: [("voxels of the world", GUIDE_WORLD[0] * GUIDE_WORLD[1] * GUIDE_WORLD[2], 1 << 32),
               ("largest index inside the world", max(h for h in GUIDE_HITS if h < GUIDE_WORLD[0] * GUIDE_WORLD[1] * GUIDE_WORLD[2]), 1 << 32),
               ("indices outside the world", sum(h >= GUIDE_WORLD[0] * GUIDE_WORLD[1] * GUIDE_WORLD[2] for h in GUIDE_HITS), 1),
               ("negative indices", sum(h < 0 for h in GUIDE_HITS), 1),
               ("side", max(max(f) for f in GUIDE_FRAMES), c["dn_max_side"] - 1)])

# ---- 11. PARTIAL_OVERLAP
OVERLAP_FRAME = (65, 33)
OVERLAP_ITERATIONS = (1, 2)


def overlap_shifts(W):
    """bytes from d_color_in to d_color_out: a row up and down, a pixel up and down"""
    return (12 * W, -12 * W, 12, -12)


PARTIAL_OVERLAP = Case(
    "partial_overlap", "vxrt_denoise.hip: denoise_frame's pack launch when one iteration's output overlaps its input in part",
    dict(frame=OVERLAP_FRAME, iterations=OVERLAP_ITERATIONS),
    lambda c: [("bytes of a frame", 12 * OVERLAP_FRAME[0] * OVERLAP_FRAME[1], max(abs(s) for s in overlap_shifts(OVERLAP_FRAME[0]))),
               ("smallest shift", min(abs(s) for s in overlap_shifts(OVERLAP_FRAME[0])), 0),
               ("iterations that need no pack launch", max(OVERLAP_ITERATIONS), 1),
               ("iterations", c["dn_max_iterations"], max(OVERLAP_ITERATIONS) - 1)])

REGION_CASES = [GRID_Y_ALONG_Z, GRID_Y_ALONG_ROWS, ZSTEPS_LADDER, ROW_MAPPINGS]
SURFACE_CASES = [SCAN_SHARE, CHECKERBOARD_COUNTS]
DENOISE_CASES = [THIN_FRAMES_CASE, PIXEL_LIMIT, SPECIAL_VALUES, GUIDE_KEYS_LARGE_WORLD, PARTIAL_OVERLAP]
LAUNCH_CASES = REGION_CASES + SURFACE_CASES + DENOISE_CASES


# ---- references computed once and shared by the tests of a session (read-only)
@functools.lru_cache(maxsize=None)
def denoised(W, H, k, iterations):
    """the restatement's result of the random frame (W, H) after `iterations` iterations with colour scale k; the chain is
    kept, so that a longer one goes on from a shorter one"""
    c, keys = RD.random_frame(W, H)
    out = RD.iterate_np(denoised(W, H, k, iterations - 1), keys, 1 << (iterations - 1), k) if iterations else np.ascontiguousarray(c, np.float32)
    out.setflags(write=False)
    return out
