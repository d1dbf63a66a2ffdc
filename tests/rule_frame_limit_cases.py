"""Rule and frame limit cases: calls of vxrt_apply_rule, vxrt_reproject_frame and vxrt_light_frame whose shapes reach the code
that only runs past a launch cap or at the largest values the contract allows, their special operands, and worlds whose three
sides differ.  Shared by tests/test_rule_frame_limits_host.py, which holds every case to the cap it must exceed, the launch
arithmetic below to the figures worked out by hand and every identity below to the restatements (tests/ref_rule.py,
tests/ref_reproject.py, tests/ref_light_frame.py) at small sizes, and tests/test_gpu_rule_frame_limits.py, which runs the cases
on the device.

The caps live in voxelengine_amd/csrc; read_caps() reads them with regexes that must match exactly once:
- the rule's planes (vxrt_rule.hpp: rule_layout) have np = ceil((dims[0] + 2 h) / 32) * (dims[1] + 2 h) * (dims[2] + 2 h) words,
  h = 1 (BOX) or `iterations` (WORLD); k_rule_setup and k_rule_round take one lane per plane word in workgroups of 256, and
  grid_2d (vxrt_region.hpp) takes the launch to a second grid axis past 2^20 workgroups; the workgroups it adds to fill the
  last grid row must write nothing;
- k_rule_output (vxrt_rule.hip) is a grid-stride launch of `few` workgroups over tb = ceil(nb / 256) blocks of output words:
  few = tb below 128, 128 while tb / 8 < 128, tb / 8 from there on, at most 1024;
- kRuleMaxVoxels and kRuleMaxIterations bound the box and the iterations;
- the frame kernels share rp_launch_shape (vxrt_reproject.hpp): without a summary one workgroup of kRpPlain lanes per tile
  of 64 x 4 pixels, with one at most cus * kRpCountedPerCu workgroups of kRpCounted lanes whose waves walk several tiles;
  kDnMaxSide and kDnMaxPixels (vxrt_denoise.hpp) bound the frame, kLfMaxBoxVoxels (vxrt_light_frame.hpp) the light box.
Every case names the caps it must exceed.

Not reachable, so not covered:
- a start of the plane turn[1] past 2^32 bytes: the largest plane is 4 * (2^28 / 32 * 3 * 3 * (1 + 2^-23)) bytes for a row of
  2^28 voxels and 2^30 + 32 bytes for case 1, so turn[1] starts at 3 * 2^30 + 768 at the most; its END lies past 2^32 in
  case 1 (so does the workspace's), which is what the case states;
- grid_2d's second axis in k_rule_output: the launch is capped at 1024 workgroups;
- a world of three different sides at brick edges 16 and 32 with sides of 256, 64 and 128 voxels: the tables hold whole tiles
  of 8 x 8 x 8 cells, so every side is a multiple of 8 * edge.  SIDES_WORLDS has that world at edge 8 and the smallest
  worlds of sides in the same order (X > Z > Y, 24 x 8 x 16 cells) at the other two.

The second box of case 2 is two rows of 2^27 - 59 voxels, the widest rows with five voxels in their last word of which two
make a box within kRuleMaxVoxels (two rows of 2^27 + 5 voxels are 2^28 + 10 voxels: refused).

Identities for the cases too large for the restatement, each held against it at small sizes by the host test:
clipped_z (a box far longer than the world along z: inside z in [-n, Z + n) the bits are those of the box cut to that range,
0 elsewhere, the summary the cut box's), row_window (a box far longer than the world along x: the words that hold the world
are those of the box cut to whole words around it) and checker_summary (a rule that is born on every count from 1 on and
never survives turns the parity checkerboard into its complement at every step); near_box (a light box cut to the cells next
to the 64^3 world lights a frame alike); and, for the frame of nearly kDnMaxPixels pixels, inputs that are a hash of the pixel
index (evaluated by torch on the device and by numpy here) with the restatements evaluated on bands of rows (rows=(y0, y1)),
which the host test holds to be slices of the whole frame's evaluation.

The axis fields 3 and 31 of case 8 go to vxrt_light_frame alone: its contract reads an axis field above 2 as axis 2, that of
vxrt_reproject_frame takes guide keys (axis 0 .. 2) and says nothing of others.  The two restatements of either kernel agree
on every special operand of case 8."""
from __future__ import annotations

import functools
import os
import re
from types import SimpleNamespace

import numpy as np

from tests import light_frame_cases as LC
from tests import ref_denoise as RD
from tests import ref_light_frame as LF
from tests import ref_rule as R
from tests.launch_limit_cases import CAP_SOURCES as _LAUNCH_SOURCES
from tests.read_limit_cases import (CHECKER_WORLD, GUIDE_FRAMES, GUIDE_HITS, GUIDE_WORLD, SPECIALS, THIN_FRAMES, Case, ceil_div, guide_hits,
                                    small_world, special_frame)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = "voxelengine_amd/csrc/"
_shift = lambda s: 1 << int(s)
F32 = np.float32
NONE = ((R.INT_MAX,) * 3, (R.INT_MIN,) * 3)  # the changed box of a call that changed nothing

_FEW = r"few = tb / %su < %su \? \(tb < %su \? tb : %su\) : tb / %su;"
CAP_SOURCES = {  # name: (file, regex whose group 1 is the value, value from the group); each must match exactly once
    "grid_2d_x": _LAUNCH_SOURCES["grid_2d_x"],
    "rule_max_voxels": (_CSRC + "vxrt_rule.hpp", r"constexpr uint64_t kRuleMaxVoxels = 1ull << (\d+);", _shift),
    "rule_max_iterations": (_CSRC + "vxrt_rule.hpp", r"constexpr int32_t kRuleMaxIterations = (\d+);", int),
    "rule_out_floor": (_CSRC + "vxrt_rule.hip", _FEW % (r"\d+", r"(\d+)", r"\1", r"\1", r"\d+"), int),
    "rule_out_share": (_CSRC + "vxrt_rule.hip", _FEW % (r"(\d+)", r"\d+", r"\d+", r"\d+", r"\1"), int),
    "rule_out_cap": (_CSRC + "vxrt_rule.hip", r"dim3\(\(unsigned\)\(few < (\d+)u \? few : \1u\)\)", int),
    "rp_plain": (_CSRC + "vxrt_reproject.hpp", r"constexpr uint32_t kRpPlain = (\d+)u, kRpCounted = \d+u, kRpCountedPerCu = \d+u;", int),
    "rp_counted": (_CSRC + "vxrt_reproject.hpp", r"constexpr uint32_t kRpPlain = \d+u, kRpCounted = (\d+)u, kRpCountedPerCu = \d+u;", int),
    "rp_counted_per_cu": (_CSRC + "vxrt_reproject.hpp", r"constexpr uint32_t kRpPlain = \d+u, kRpCounted = \d+u, kRpCountedPerCu = (\d+)u;", int),
    "rp_max_history": (_CSRC + "vxrt_reproject.hpp", r"constexpr int32_t kRpMaxHistory = (\d+);", int),
    "lf_max_box_voxels": (_CSRC + "vxrt_light_frame.hpp", r"constexpr uint64_t kLfMaxBoxVoxels = 1ull << (\d+);", _shift),
    "dn_max_side": (_CSRC + "vxrt_denoise.hpp", r"constexpr uint32_t kDnMaxSide = (\d+)u;", int),
    "dn_max_pixels": (_CSRC + "vxrt_denoise.hpp", r"constexpr uint64_t kDnMaxPixels = 1ull << (\d+);", _shift),
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


# ---- the launch arithmetic of vxrt_apply_rule (vxrt_rule.hpp: rule_layout; vxrt_rule.hip: apply_rule), restated
def rule_layout(dims, h):
    """the halo box, the words of a halo row, of a plane, of an output row and of the output, and the workspace's byte offsets"""
    hd = tuple(int(d) + 2 * h for d in dims)
    wh, mw = ceil_div(hd[0], 32), ceil_div(int(dims[0]), 32)
    words = wh * hd[1] * hd[2]
    plane = ceil_div(4 * words, 256) * 256
    return SimpleNamespace(hd=hd, wh=wh, np=words, mw=mw, nb=mw * int(dims[1]) * int(dims[2]), w0=0, free=plane, turn=(2 * plane, 3 * plane),
                           total=4 * plane)


def rule_launch(dims, h, caps):
    """the grid of k_rule_setup and k_rule_round (blocks, gx, gy, surplus) and of k_rule_output (tb, few, grid, regime)"""
    L = rule_layout(dims, h)
    blocks = ceil_div(L.np, 256)
    gx = min(blocks, caps["grid_2d_x"])
    gy = ceil_div(blocks, gx)
    tb = ceil_div(L.nb, 256)
    floor, share = caps["rule_out_floor"], caps["rule_out_share"]
    few = (tb if tb < floor else floor) if tb // share < floor else tb // share
    regime = "share" if tb // share >= floor else "all" if tb < floor else "floor"
    return SimpleNamespace(blocks=blocks, gx=gx, gy=gy, surplus=gx * gy - blocks, tb=tb, few=few, grid=min(few, caps["rule_out_cap"]), regime=regime,
                           strides=ceil_div(tb, min(few, caps["rule_out_cap"])), layout=L)


def lively(rng, world, o, d, nb, scope, n, outside, mask=None):
    """random tables under which, by the restatement, voxels of the box are born and die"""
    for _ in range(50):
        rule = R.random_rule(rng, nb, n, scope, outside)
        s = R.apply_rule(world, o, d, rule, mask)["summary"]
        if s[2] > 0 and s[3] > 0:
            return rule
    raise AssertionError("no lively rule for %r %r" % (o, d))


def _frozen(want):
    want["bits"].setflags(write=False)
    return want


# ---- 1. PLANES_ON_GRID_Y: one voxel wide, two high, 2^26 slices, the world's columns inside
PLANES_ORIGIN, PLANES_DIMS, PLANES_ITERATIONS = (37, 11, -100), (1, 2, 1 << 26), 2
# the same box ending at the world's last slice: the plane words of that slice and of the halo slice behind it are the eight
# words of the second grid row (a launch that dropped blockIdx.y would leave the first origin's result as it is: everything
# the second grid row computes there lies outside the world and is cut from the output)
PLANES_ORIGINS = (PLANES_ORIGIN, (37, 11, 64 - (1 << 26)))


def clipped_z(origin, dims, world_z, n):
    """the box cut to the slices z in [-n, world_z + n): (origin, dims, the cut's first slice counted from the box's)"""
    z0, z1 = max(origin[2], -n), min(origin[2] + dims[2], world_z + n)
    assert z0 < z1
    return (origin[0], origin[1], z0), (dims[0], dims[1], z1 - z0), z0 - origin[2]


@functools.lru_cache(maxsize=None)
def planes_expected(outside, k=0):
    """(the rule, the restatement's result on the cut box, the cut's first slice) at PLANES_ORIGINS[k]: BOX, N26, two iterations"""
    world = small_world()
    o, d, first = clipped_z(PLANES_ORIGINS[k], PLANES_DIMS, world.shape[2], PLANES_ITERATIONS)
    rule = lively(np.random.default_rng(61 + outside + 2 * k), world, o, d, R.N26, R.BOX, PLANES_ITERATIONS, outside)
    return rule, _frozen(R.apply_rule(world, o, d, rule)), first


def _planes(c):
    return rule_launch(PLANES_DIMS, 1, c)


PLANES_ON_GRID_Y = Case(
    "planes_on_grid_y", "vxrt_rule.hip: k_rule_setup and k_rule_round on grid_2d's second axis, surplus workgroups, a workspace past 2^32 bytes",
    dict(world=(64, 64, 64, 8), origins=PLANES_ORIGINS, dims=PLANES_DIMS, iterations=PLANES_ITERATIONS),
    lambda c: [("workgroups", _planes(c).blocks, c["grid_2d_x"]),
               ("surplus workgroups", _planes(c).surplus, 0),
               ("workspace bytes", _planes(c).layout.total, 1 << 32),
               ("end of turn[1] in bytes", _planes(c).layout.turn[1] + 4 * _planes(c).layout.np, 1 << 32),
               ("output workgroups before the cap", _planes(c).few, c["rule_out_cap"]),
               ("slices before the world", -PLANES_ORIGIN[2], PLANES_ITERATIONS),
               ("plane word of the world's last slice at the second origin", (63 - PLANES_ORIGINS[1][2] + 1) * 4, 256 * c["grid_2d_x"] - 1)])

# ---- 2. LONG_ROWS: rows of 2^23 and 2^22 words
ROWS_BOXES = (((64 + 3 - (1 << 28), 10, 20), (1 << 28, 1, 1)), ((-7, 10, 20), ((1 << 27) - 59, 2, 1)))
ROWS_WINDOW = 4  # the words of a row that hold the world's 64 voxels: the last ones of the first box, the first ones of the second


def row_window(origin, dims, first, words):
    """the box cut to the words first .. first + words - 1 of every row (a box whose origin is moved up by whole words
    returns the words of the row from there on: the region layout of include/vxrt.h): (origin, dims)"""
    x0 = origin[0] + 32 * first
    return (x0,) + tuple(origin[1:]), (min(32 * words, origin[0] + dims[0] - x0),) + tuple(dims[1:])


def rows_first_word(k):
    return ceil_div(ROWS_BOXES[k][1][0], 32) - ROWS_WINDOW if k == 0 else 0


@functools.lru_cache(maxsize=None)
def rows_expected(k, outside):
    """(the rule, the restatement's result on the window's box): BOX, N18, one iteration"""
    world = small_world()
    o, d = row_window(*ROWS_BOXES[k], rows_first_word(k), ROWS_WINDOW)
    assert o[0] < 0 and o[0] + d[0] > world.shape[0]  # the world's voxels of the rows lie strictly inside the window
    rule = lively(np.random.default_rng(63 + 2 * k + outside), world, o, d, R.N18, R.BOX, 1, outside)
    return rule, _frozen(R.apply_rule(world, o, d, rule))


LONG_ROWS = Case(
    "long_rows", "vxrt_rule.hpp: rule_row's carries, rule_gather and rule_span along rows of 2^23 words",
    dict(world=(64, 64, 64, 8), boxes=ROWS_BOXES),
    lambda c: [("words per halo row", rule_layout(ROWS_BOXES[0][1], 1).wh, (1 << 23) - 1),
               ("words per halo row of the second box", rule_layout(ROWS_BOXES[1][1], 1).wh, (1 << 22) - 2),
               ("voxels of the first box", ROWS_BOXES[0][1][0], c["rule_max_voxels"] - 1),
               ("voxels before the world", -ROWS_BOXES[0][0][0], (1 << 28) - 128),
               ("output workgroups before the cap", rule_launch(ROWS_BOXES[0][1], 1, c).few, c["rule_out_cap"]),
               ("ragged last word of the second box", ROWS_BOXES[1][1][0] % 32, 0)])

# ---- 3. OUTPUT_REGIMES: few = tb, the floor of 128, tb / 8 and the cap of 1024
REGIME_WORLD = (128, 128, 128, 16)
REGIME_ORIGIN, REGIME_DIMS = (60, -286, -290), (1, 700, 700)
REGIME_RULES = ((R.N26, R.BOX, 2, 1), (R.N18, R.WORLD, 2, 0))  # (neighbourhood, scope, iterations, outside)
REGIME_SMALL = (37, 9, 5)      # a box of tests/test_gpu_rule.py (test_many_halo_rows_and_the_ends_of_int32): few = tb = 1
REGIME_FLOOR = (1, 300, 300)   # another box of that test: tb = 352, few = 128


@functools.lru_cache(maxsize=None)
def regime_world():
    w = R.gradient_world(np.random.default_rng(65), REGIME_WORLD[:3])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def regime_expected(k):
    nb, scope, n, outside = REGIME_RULES[k]
    rule = lively(np.random.default_rng(66 + k), regime_world(), REGIME_ORIGIN, REGIME_DIMS, nb, scope, n, outside)
    return rule, _frozen(R.apply_rule(regime_world(), REGIME_ORIGIN, REGIME_DIMS, rule))


OUTPUT_REGIMES = Case(
    "output_regimes", "vxrt_rule.hip: k_rule_output's grid: tb / 8 workgroups, each lane on more than one word",
    dict(world=REGIME_WORLD, origin=REGIME_ORIGIN, dims=REGIME_DIMS, rules=REGIME_RULES),
    lambda c: [("workgroups of the middle branch", rule_launch(REGIME_DIMS, 1, c).tb // c["rule_out_share"], c["rule_out_floor"] - 1),
               ("the cap over the middle branch's workgroups", c["rule_out_cap"], rule_launch(REGIME_DIMS, 1, c).few),
               ("words in turn of a lane", rule_launch(REGIME_DIMS, 1, c).strides, c["rule_out_share"] - 1),
               ("workgroups before the cap in case 4", rule_launch(CHECKER_WORLD[:3], 1, c).few, c["rule_out_cap"]),
               ("the floor over a small box's blocks", c["rule_out_floor"], rule_launch(REGIME_SMALL, 1, c).tb),
               ("blocks of a box at the floor", rule_launch(REGIME_FLOOR, 1, c).tb, c["rule_out_floor"] - 1),
               ("the floor over that box's share", c["rule_out_floor"], rule_launch(REGIME_FLOOR, 1, c).tb // c["rule_out_share"])])

# ---- 4. COUNTERS_AT_2_28: the parity checkerboard of tests/read_limit_cases.py, every voxel changing at every step
COUNTER_RUNS = ((R.BOX, 1), (R.BOX, 2), (R.WORLD, 3), (R.WORLD, 16))  # (scope, iterations)
NEIGHBOURHOODS = (R.N6, R.N18, R.N26)


def flip_rule(nb, scope, n, outside):
    """born on every count from 1 on, never surviving: an empty voxel of the board has 6 (N6, N18: its edge neighbours have
    its own parity) or 14 (N26) solid neighbours, at the world's faces at least 3, so every step gives the complement"""
    return R.RefRule(nb, R.bits_of(range(1, R.COUNT[nb] + 1)), 0, n, scope, outside)


def checker_summary(dims, n):
    """the summary of the flip rule on the board's own box after n steps"""
    v = dims[0] * dims[1] * dims[2]
    assert v % 2 == 0
    if n % 2:
        return (v // 2, v // 2, v // 2, v // 2, v, (0, 0, 0), tuple(d - 1 for d in dims))
    return (v // 2, v // 2, 0, 0, v, *NONE)


COUNTERS_AT_2_28 = Case(
    "counters_at_2_28", "vxrt_rule.hip: k_rule_output's tally and the summary's counters at 2^28, the cap of 1024 workgroups",
    dict(world=CHECKER_WORLD, runs=COUNTER_RUNS),
    lambda c: [("voxels", CHECKER_WORLD[0] * CHECKER_WORLD[1] * CHECKER_WORLD[2], c["rule_max_voxels"] - 1),
               ("changed_last", checker_summary(CHECKER_WORLD[:3], 1)[4], c["rule_max_voxels"] - 1),
               ("iterations", max(n for _, n in COUNTER_RUNS), c["rule_max_iterations"] - 1),
               ("workgroups before the cap", rule_launch(CHECKER_WORLD[:3], 1, c).few, c["rule_out_cap"]),
               ("words in turn of a lane", rule_launch(CHECKER_WORLD[:3], 1, c).strides, 31)])

# ---- 5. THREE_SIDES: worlds whose three sides differ
SIDES_WORLDS = {8: (256, 64, 128), 16: (384, 128, 256), 32: (768, 256, 512)}  # brick edge: (X, Y, Z)
SIDES_SCOPES = ((R.BOX, 2), (R.WORLD, 2))


@functools.lru_cache(maxsize=None)
def sides_world(factor):
    """gradient density along x (tests/ref_rule.py: gradient_world), drawn in binary32 for the larger worlds"""
    shape = SIDES_WORLDS[factor]
    ramp = ((np.arange(shape[0]) + 0.5) / shape[0]).astype(F32)
    w = np.random.default_rng(67 + factor).random(shape, dtype=F32) < ramp[:, None, None]
    w.setflags(write=False)
    return w


def sides_boxes(factor):
    """the world's own box grown by five voxels over all six faces (edge 8; at the larger edges, where the restatement of
    that box would take minutes, a box over the three low faces), a box over the y-hi face alone, one over the z-hi face
    alone (by another amount) and one over the three far faces (at the larger edges with more of it inside the world, whose
    last voxels along x are nearly all solid)"""
    X, Y, Z = SIDES_WORLDS[factor]
    first = ((-5, -5, -5), (X + 10, Y + 10, Z + 10)) if factor == 8 else ((-5, -5, -5), (70, 40, 30))
    return (first, ((X // 2 - 28, Y - 14, Z // 2 - 24), (33, 30, 20)), ((X // 2 - 28, Y // 2 - 12, Z - 18), (31, 20, 40)),
            ((X - 6, Y - 4, Z - 8), (40, 9, 20)) if factor == 8 else ((X - 24, Y - 6, Z - 12), (40, 9, 20)))


def sides_overhang(factor, k):
    """by how many voxels box k passes the faces (x-lo, x-hi, y-lo, y-hi, z-lo, z-hi), 0 where it does not"""
    o, d = sides_boxes(factor)[k]
    return tuple(v for a, n, w in zip(o, d, SIDES_WORLDS[factor]) for v in (max(-a, 0), max(a + n - w, 0)))


@functools.lru_cache(maxsize=None)
def sides_expected(factor, k, s):
    """box k under scope SIDES_SCOPES[s]: (origin, dims, rule, mask, the restatement's result); the neighbourhoods and
    `outside` spread over the boxes, the BOX calls with a mask, the tables lively"""
    world = sides_world(factor)
    o, d = sides_boxes(factor)[k]
    scope, n = SIDES_SCOPES[s]
    nb, outside = NEIGHBOURHOODS[(k + s) % 3], (k + s) & 1
    rng = np.random.default_rng(1000 * factor + 10 * k + s)
    mask = rng.random(d) < 0.8 if scope == R.BOX else None
    if d[0] * d[1] * d[2] > 200000:  # (lively on a small box at the world's centre; the host test holds it to be lively on the box)
        rule = lively(rng, world, tuple(v // 2 - 8 for v in world.shape), (16, 16, 16), nb, scope, n, outside)
    else:
        rule = lively(rng, world, o, d, nb, scope, n, outside, mask)
    if mask is not None:
        mask.setflags(write=False)
    return o, d, rule, mask, _frozen(R.apply_rule(world, o, d, rule, mask))


THREE_SIDES = Case(
    "three_sides", "vxrt_rule.hpp: the in-world masks of rule_setup_lane and rule_output_lane on worlds with X > Z > Y",
    dict(worlds=SIDES_WORLDS, scopes=SIDES_SCOPES),
    lambda c: [("distinct sides of a world", min(len(set(w)) for w in SIDES_WORLDS.values()), 2),
               ("a box past y-hi that stays below the world's z side", SIDES_WORLDS[8][2], max(o[1] + d[1] for o, d in sides_boxes(8)[1:2])),
               ("first slice of the z-hi box, past the world's y side", sides_boxes(8)[2][0][2], SIDES_WORLDS[8][1]),
               ("overhang over y-hi alone", min(sides_overhang(f, 1)[3] for f in SIDES_WORLDS), 0),
               ("overhang over z-hi alone", min(sides_overhang(f, 2)[5] for f in SIDES_WORLDS), 0),
               ("faces the first box of edge 8 passes", sum(v > 0 for v in sides_overhang(8, 0)), 5),
               ("brick edges", len(SIDES_WORLDS), 2)])

RULE_CASES = [PLANES_ON_GRID_Y, LONG_ROWS, OUTPUT_REGIMES, COUNTERS_AT_2_28, THREE_SIDES]

# ---- the launch of the frame kernels (vxrt_reproject.hpp: rp_launch_shape, rp_wave_pixel), restated
NOMINAL_CUS = 256  # the compute units the cases' reach lines assume; the GPU test restates them for the device it runs on


def frame_launch(W, H, summary, cus, caps):
    """tiles of 64 x (kRpPlain / 64) pixels, the lanes of a workgroup, the workgroups, which of `need` and the device's
    share binds (counted launch) and the tiles a wave walks"""
    rows = caps["rp_plain"] // 64
    across, down = ceil_div(W, 64), ceil_div(H, rows)
    tiles = across * down
    if not summary:
        return SimpleNamespace(across=across, down=down, tiles=tiles, block=caps["rp_plain"], grid=tiles, binds="tiles", per_wave=1)
    groups = max(caps["rp_counted"] // caps["rp_plain"], 1)  # tiles a workgroup holds at a time
    need, most = ceil_div(tiles, groups), max(cus, 1) * caps["rp_counted_per_cu"]
    grid = min(need, most)
    return SimpleNamespace(across=across, down=down, tiles=tiles, block=caps["rp_counted"], grid=grid, binds="need" if need < most else "cus",
                           per_wave=ceil_div(tiles, grid * groups))


# ---- 6. THIN_FRAMES of tests/read_limit_cases.py through vxrt_reproject_frame and vxrt_light_frame
THIN_HOST_CUS = 3  # the compute units the host harnesses run the thin frames with: about 340 and 2700 tiles a wave


def thin_pose():
    """an orthonormal pose looking down at a slant.  The poses of tests/ref_reproject.py are orthogonal to a few percent
    only, which a frame 65535 pixels wide and 5 high turns into thousands of rows: every pixel would leave the frame"""
    fwd = np.array([0.3, -0.9, 0.2])
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.1, 0.2, 0.95])
    right /= np.linalg.norm(right)
    return fwd, np.cross(right, fwd), right


@functools.lru_cache(maxsize=None)
def thin_reproject(W, H, ortho):
    """(tests/ref_reproject.py's random case under thin_pose and a previous camera moved without turning -- by 0.7 and 1.3
    pixels of the ortho window, by hundredths of a voxel in perspective --, the restatement's records and summary)"""
    from tests import ref_reproject as T
    case = dict(T.random_case(W, H, ortho))
    pos = np.asarray(case["cur"][0], np.float64)
    fwd, up, right = thin_pose()
    px, py = 2 * T.ORTHO_SIZE[0] * (W / H) / W, 2 * T.ORTHO_SIZE[1] / H
    move = 0.7 * px * right + 1.3 * py * up if ortho else 0.02 * right + 0.01 * up
    case["cur"] = tuple(np.asarray(v, F32) for v in (pos, fwd, up, right))
    case["prev"] = tuple(np.asarray(v, F32) for v in (pos + move, fwd, up, right))
    rec, summary = T.run_case(case)
    rec.setflags(write=False)
    return case, rec, summary


@functools.lru_cache(maxsize=None)
def thin_light(W, H, ortho):
    """(the random case of tests/light_frame_cases.py, the restatement's colours, terms and summary)"""
    case = LC.random_case(W, H, ortho)
    color, terms, summary = LC.run_case(case)[:3]
    color.setflags(write=False)
    terms.setflags(write=False)
    return case, color, terms, summary


THIN_FRAMES_CASE = Case(
    "thin_frames", "vxrt_reproject.hpp: rp_launch_shape and rp_wave_pixel on frames of kDnMaxSide pixels a side, counted and plain",
    dict(frames=THIN_FRAMES, cameras=("perspective", "ortho")),
    lambda c: [("side", max(f), c["dn_max_side"] - 1) for f in THIN_FRAMES] +
              [("tiles across", frame_launch(*THIN_FRAMES[0], False, NOMINAL_CUS, c).across, 1023),
               ("tile rows", frame_launch(*THIN_FRAMES[1], False, NOMINAL_CUS, c).down, 16383),
               ("tile's width over the frame's", 64, THIN_FRAMES[1][0]),
               ("tiles a wave of the counted launch walks", frame_launch(*THIN_FRAMES[1], True, NOMINAL_CUS, c).per_wave, 7),
               ("workgroups of the plain launch", frame_launch(*THIN_FRAMES[1], False, NOMINAL_CUS, c).grid, 16383)])

# ---- 11. LIGHT_THREE_SIDES: vxrt_light_frame on the worlds of case 5
LIGHT_SIDES_FRAME = (160, 96)


def light_sides_box(factor):
    """a light box that passes the y-hi face by 16 voxels and the z-hi face by 32"""
    X, Y, Z = SIDES_WORLDS[factor]
    return ((X // 2 - 30, Y - 24, Z - 38), (60, 40, 70))


@functools.lru_cache(maxsize=None)
def light_sides_case(factor, ortho):
    """tests/light_frame_cases.py's random_case on the world of case 5 at brick edge `factor`: a camera inside the world near
    the light box looking down at a slant, hit indices on the pixel's own ray, anywhere in the world, on each of the
    world's six boundary layers, beyond the world and -1; (the case, the restatement's colours, terms, summary and info)"""
    W, H = LIGHT_SIDES_FRAME
    world = sides_world(factor)
    dims = np.array(world.shape)
    X, Y, Z = (int(v) for v in dims)
    box = light_sides_box(factor)
    rng = np.random.default_rng(71 * factor + int(ortho))
    levels = rng.integers(0, 256, box[1], dtype=np.uint8)
    color, _ = RD.random_frame(W, H, factor)
    cam = tuple(np.asarray(v, F32) for v in ((X / 2 - 10.5, Y - 12.75, Z - 40.25), (0.3, -0.9, 0.2), (0.1, 0.2, 0.95), (0.95, 0.3, -0.1)))
    o, d = RD.primary_rays(W, H, *cam, ortho=ortho, ortho_size=LC.ORTHO_SIZE)
    along = (o.astype(np.float64) + rng.uniform(2.0, 40.0, (H, W, 1)) * d).astype(np.int64)
    on_ray = ((along >= 0) & (along < dims)).all(-1)
    along = np.clip(along, 0, dims - 1)
    near = np.array(box[0]) - 8 + np.stack([rng.integers(0, n + 16, (H, W)) for n in box[1]], -1)  # around the light box
    anywhere = np.where(rng.random((H, W, 1)) < 0.5, np.clip(near, 0, dims - 1), np.stack([rng.integers(0, n, (H, W)) for n in dims], -1))
    edge = anywhere.copy()
    side = rng.integers(0, 6, (H, W))
    np.put_along_axis(edge, (side >> 1)[..., None], np.where(side & 1, dims[side >> 1] - 1, 0)[..., None], -1)
    index = lambda v: v[..., 0] + X * (v[..., 1] + Y * v[..., 2])
    pick = rng.random((H, W))
    hit = np.where(on_ray, index(along), index(anywhere))
    hit = np.where((pick >= 0.4) & (pick < 0.6), index(anywhere), hit)
    hit = np.where((pick >= 0.6) & (pick < 0.85), index(edge), hit)
    hit = np.where((pick >= 0.85) & (pick < 0.9), X * Y * Z + rng.integers(0, 3, (H, W)) * (1 << 40), hit)
    hit = np.where(pick >= 0.9, -1, hit).astype(np.int64)
    keys = RD.keys_np(hit, world.shape, o, d)
    for a in (levels, color, hit, keys):
        a.setflags(write=False)
    case = dict(world=world, levels=levels, box=box, color=color, hit=hit, keys=keys, cam=cam, ortho=ortho, ortho_size=LC.ORTHO_SIZE,
                params=dict(LC.PARAMS), edge_side=np.where((pick >= 0.6) & (pick < 0.85), side, -1))
    out = LC.run_case(case)
    for a in out[:2]:
        a.setflags(write=False)
    return (case,) + tuple(out)


def _light_box_overhang(factor):
    (o, d), w = light_sides_box(factor), SIDES_WORLDS[factor]
    return tuple(a + n - s for a, n, s in zip(o, d, w))


LIGHT_THREE_SIDES = Case(
    "light_three_sides", "vxrt_light_frame.hpp: lf_solid's bounds and cell index on worlds with X > Z > Y",
    dict(worlds=SIDES_WORLDS, frame=LIGHT_SIDES_FRAME),
    lambda c: [("distinct sides of a world", min(len(set(w)) for w in SIDES_WORLDS.values()), 2),
               ("the light box past y-hi", min(_light_box_overhang(f)[1] for f in SIDES_WORLDS), 0),
               ("the light box past z-hi, by another amount", min(_light_box_overhang(f)[2] - _light_box_overhang(f)[1] for f in SIDES_WORLDS), 0),
               ("the world's x side over the light box", min(-_light_box_overhang(f)[0] for f in SIDES_WORLDS), 0),
               ("the camera's height over the smallest world's y side in z", SIDES_WORLDS[8][2] - 41, SIDES_WORLDS[8][1]),
               ("brick edges", len(SIDES_WORLDS), 2)])


# ---- 10. LIGHT_BOX_LIMITS: the light box at the largest size and the lowest origin the contract allows
LIGHT_BOXES = (((70 - (1 << 28), 30, 30), (1 << 28, 1, 1)),        # a row: its last 72 bytes lie at x in -2 .. 69
               ((0, 0, 64 - 65536), (64, 64, 65536)),               # kLfMaxBoxVoxels voxels: its last 66 slices lie at z in -2 .. 63
               ((-(1 << 31), 0, 0), (1 << 28, 1, 1)))               # no cell of or next to the world
LIGHT_BOX_FRAME = (160, 96)
LIGHT_BOX_POISON = 0x5D  # every byte of a light box that no cell near the world names
NEAR = (-2, 66)          # the cells a hit voxel of the 64^3 world can name lie in -1 .. 64 on every axis


def near_box(box):
    """the part of a light box that a cell next to the 64^3 world can name, or None: every cell a pixel looks up lies in
    -1 .. 64 on every axis, so the light on a frame does not change when the box is cut to NEAR and the levels to the
    slice of it; (origin, dims, the slice's first cell counted from the box's)"""
    lo = [max(o, NEAR[0]) for o in box[0]]
    hi = [min(o + d, NEAR[1]) for o, d in zip(*box)]
    if any(a >= b for a, b in zip(lo, hi)):
        return None
    return tuple(lo), tuple(b - a for a, b in zip(lo, hi)), tuple(a - o for a, o in zip(lo, box[0]))


def aimed_case(W, H, world, box, ortho, seed, levels=True):
    """a light-on-frames case whose hit voxels have their front cells in `box` (cut to the cells near the world), on its
    faces and up to two cells outside it: keys made for the purpose (any axis, either side), the rays of the camera of
    tests/light_frame_cases.py; levels random bytes over the cut box"""
    rng = np.random.default_rng(seed)
    dims = np.array(world.shape)
    X, Y, Z = (int(v) for v in dims)
    cut = near_box(box) or ((20, 20, 20), (8, 8, 8), None)
    lv = rng.integers(0, 256, cut[1], dtype=np.uint8) if levels and near_box(box) else None
    color, _ = RD.random_frame(W, H, seed)
    cam = tuple(np.asarray(v, F32) for v in ((14.5, 44.25, 20.75), (0.3, -0.9, 0.2), (0.1, 0.2, 0.95), (0.95, 0.3, -0.1)))
    front = np.array(cut[0]) - 2 + np.stack([rng.integers(0, n + 4, (H, W)) for n in cut[1]], -1)
    a = rng.integers(0, 3, (H, W))
    toward = rng.integers(0, 2, (H, W))
    v = front + np.eye(3, dtype=np.int64)[a] * np.where(toward, 1, -1)[..., None]  # (the front cell is v - e_a when toward)
    inside = ((v >= 0) & (v < dims)).all(-1)
    v = np.where(inside[..., None], v, rng.integers(0, 64, (H, W, 3)))
    plane = np.take_along_axis(v, a[..., None], -1)[..., 0] + np.where(toward, 0, 1)
    keys = ((1 << 31) | (a << 26) | (toward << 25) | plane).astype(np.uint32)
    hit = v[..., 0] + X * (v[..., 1] + Y * v[..., 2])
    pick = rng.random((H, W))
    hit = np.where(pick < 0.05, -1, np.where(pick < 0.1, X * Y * Z + 5, hit)).astype(np.int64)
    keys = np.where(pick < 0.1, 0, keys).astype(np.uint32)
    for arr in (color, hit, keys) + (() if lv is None else (lv,)):
        arr.setflags(write=False)
    return dict(world=world, levels=lv, box=(cut[0], cut[1]), color=color, hit=hit, keys=keys, cam=cam, ortho=ortho, ortho_size=LC.ORTHO_SIZE,
                params=dict(LC.PARAMS))


@functools.lru_cache(maxsize=None)
def light_box_case(k):
    """(the case with the cut box and its levels, the restatement's colours, terms, summary and info); k even perspective"""
    world = LC.random_case(8, 8, False)["world"]
    case = aimed_case(*LIGHT_BOX_FRAME, world, LIGHT_BOXES[k], bool(k & 1), 80 + k)
    out = LC.run_case(case, levels=case["levels"] is not None)
    for a in out[:2]:
        a.setflags(write=False)
    return (case,) + tuple(out)


def _box_voxels(k):
    return LIGHT_BOXES[k][1][0] * LIGHT_BOXES[k][1][1] * LIGHT_BOXES[k][1][2]


LIGHT_BOX_LIMITS = Case(
    "light_box_limits", "vxrt_light_frame.hpp: lf_level's 64-bit differences and the byte index near 2^28",
    dict(world=(64, 64, 64, 8), boxes=LIGHT_BOXES, frame=LIGHT_BOX_FRAME),
    lambda c: [("voxels of the row box", _box_voxels(0), c["lf_max_box_voxels"] - 1),
               ("voxels of the slab box", _box_voxels(1), c["lf_max_box_voxels"] - 1),
               ("index of the first byte a pixel reads in the row box", near_box(LIGHT_BOXES[0])[2][0], (1 << 28) - 73),
               ("index of the first byte a pixel reads in the slab box", 64 * 64 * near_box(LIGHT_BOXES[1])[2][2], (1 << 28) - 66 * 4096 - 1),
               ("a cell's distance from the far box's origin", -1 - LIGHT_BOXES[2][0][0], (1 << 31) - 2),
               ("a cell's distance from the row box's origin", 64 - LIGHT_BOXES[0][0][0], (1 << 28) - 7)])

# ---- 8. SPECIAL_OPERANDS of both frame kernels on the (130, 70) frame
SPECIAL_FRAME = (130, 70)
SPECIAL_N = (float("nan"), float("inf"), -1.0, 0.5, 0.99999994, 1e-40, 1.5, 65534.0, 65535.0, 65536.0, 1e30)
SPECIAL_KEYS = (0x84000000, 0x86000000, 0x89FFFFFF)  # axis 1 plane 0 from either side; axis 2 plane 0x1FFFFFF
DOWN_POSE = ((0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))  # fwd, up, right: an ortho ray has d.x == d.z == 0 exactly
# (max_history, the previous camera): as the random case's; at the surface point the frame's centre pixel shows (z == 0
# there); 1e7 voxels behind the current one; and both cameras looking straight down
SPECIAL_REPROJECT = ((1, "near"), (2, "surface"), (65535, "far"), (65535, "near"), (2, "down"))


def _sprinkle(rng, shape, values, step=0.02):
    """an index into `values` for about `step` of the elements each, -1 elsewhere"""
    pick = rng.random(shape)
    out = np.full(shape, -1)
    for i in range(len(values)):
        out[(pick >= step * i) & (pick < step * (i + 1))] = i
    return out


@functools.lru_cache(maxsize=None)
def special_reproject(ortho, k):
    """tests/ref_reproject.py's random case of the (130, 70) frame with the colours of tests/read_limit_cases.py's
    special_frame (NaN, infinities, -0.0, denormals), the same kinds in the history under matching keys, n among
    SPECIAL_N, patches of keys on plane 0 and on plane 0x1FFFFFF in both frames, and SPECIAL_REPROJECT[k]'s max_history and
    previous camera; (the case, the restatement's records and summary, the masks the reach lines count)"""
    from tests import ref_reproject as T
    W, H = SPECIAL_FRAME
    max_history, pose = SPECIAL_REPROJECT[k]
    case = dict(T.random_case(W, H, ortho))
    rng = np.random.default_rng(90 + 2 * k + int(ortho))
    keys, keys_prev, hist = case["keys"].copy(), case["keys_prev"].copy(), case["hist"].copy()
    patch = _sprinkle(rng, ((H + 3) // 4, (W + 3) // 4), SPECIAL_KEYS, 0.04)
    patch = np.kron(patch, np.ones((4, 4), np.int64))[:H, :W]
    for i, v in enumerate(SPECIAL_KEYS):
        keys[patch == i] = v
        keys_prev[patch == i] = v
    same = (keys == keys_prev) & (keys != 0)
    kind = _sprinkle(rng, (H, W), SPECIALS)
    ch = rng.integers(0, 3, (H, W))
    for i, v in enumerate(SPECIALS):
        at = same & (kind == i)
        hist[at, ch[at]] = F32(v)
    nkind = _sprinkle(rng, (H, W), SPECIAL_N)
    for i, v in enumerate(SPECIAL_N):
        hist[same & (nkind == i), 3] = F32(v)
    case.update(color=special_frame()[0], keys=keys, keys_prev=keys_prev, hist=hist, max_history=max_history)
    pos = np.asarray(case["cur"][0], np.float64)
    if pose == "down":
        case["cur"] = tuple(np.asarray(v, F32) for v in (pos,) + DOWN_POSE)
        case["prev"] = tuple(np.asarray(v, F32) for v in (pos + np.array([0.3, 0.0, -0.2]),) + DOWN_POSE)
    elif pose == "far":
        case["prev"] = (np.asarray(pos - 1e7 * np.asarray(case["cur"][1], np.float64), F32),) + tuple(case["cur"][1:])
    elif pose == "surface":
        o, d = RD.primary_rays(W, H, *case["cur"], ortho=ortho, ortho_size=case["ortho_size"])
        y, x = H // 2, W // 2
        keys[y, x] = keys_prev[y, x] = 0x84000005  # axis 1, plane 5: below the camera
        a, pl = 1, F32(5)
        t = (pl - o[y, x, a]) / d[y, x, a]
        P = o[y, x] + t * d[y, x]
        P[a] = pl
        case["prev"] = (P.astype(F32),) + tuple(case["cur"][1:])
    for arr in (keys, keys_prev, hist):
        arr.setflags(write=False)
    rec, summary = T.run_case(case)
    rec.setflags(write=False)
    return case, rec, summary, dict(same=same, kind=kind, nkind=nkind)


def _kinds(values, array, mask):
    """how many of `values` occur in `array` (binary32, bit for bit; any NaN for a NaN) where `mask` holds"""
    n = 0
    for v in values:
        v = F32(v)
        hit = np.isnan(array) if np.isnan(v) else array.view(np.uint32) == v.view(np.uint32)
        n += bool((hit & mask).any())
    return n


def _reproject_reach(c):
    lines = [("max_history", max(m for m, _ in SPECIAL_REPROJECT), c["rp_max_history"] - 1), ("the smallest max_history below 2", 2, min(m for m, _ in SPECIAL_REPROJECT))]
    for ortho in (False, True):
        case, _, summary, m = special_reproject(ortho, 0)
        hit, miss = (case["keys"] != 0)[..., None], (case["keys"] == 0)[..., None]
        lines += [("kinds of special colours under hit keys", _kinds(SPECIALS, case["color"], hit), len(SPECIALS) - 1),
                  ("kinds of special colours under miss keys", _kinds(SPECIALS, case["color"], miss), len(SPECIALS) - 1),
                  ("kinds of special history colours under matching keys", _kinds(SPECIALS, case["hist"][..., :3], m["same"][..., None]), len(SPECIALS) - 1),
                  ("kinds of n under matching keys", _kinds(SPECIAL_N, case["hist"][..., 3], m["same"]), len(SPECIAL_N) - 1),
                  ("special keys in both frames", sum(bool(((case["keys"] == v) & m["same"]).any()) for v in SPECIAL_KEYS), len(SPECIAL_KEYS) - 1),
                  ("reused pixels", summary[1], 1000)]
    return lines


SPECIAL_REPROJECT_CASE = Case(
    "special_reproject", "vxrt_reproject.hpp: rp_pixel on NaN, infinite, negative-zero and denormal colours and history, every kind of n, the ends of the plane field",
    dict(frame=SPECIAL_FRAME, runs=SPECIAL_REPROJECT), _reproject_reach)

SPECIAL_LIGHT_PARAMS = (dict(sky_floor=0.0, block_color=(0.0, 0.0, 0.0), ao_curve=(0.0, 0.0, 0.0, 0.0), outside_level=0),
                        dict(sky_floor=1.0, block_color=(3e38, 3e38, 3e38), ao_curve=(0.0, 1.0, 2.0, 3e38), outside_level=0xFF))
SPECIAL_LIGHT = ((0, LF.SMOOTH | LF.OCCLUSION, "slant"),) + tuple((1, f, "slant") for f in LC.FLAG_SETS) + ((1, LF.SMOOTH | LF.OCCLUSION, "down"),)
SPECIAL_AXES = (3, 31)


@functools.lru_cache(maxsize=None)
def special_light(ortho, k):
    """tests/light_frame_cases.py's random case of the (130, 70) frame with special_frame's colours, keys whose axis field
    is 3 or 31 in place of 2 (read as axis 2), whose plane field is 0 or 0x1FFFFFF, SPECIAL_LIGHT[k]'s parameters and flags,
    and (pose "down", ortho) a camera whose rays have d.x == d.z == 0: (the case, colours, terms, summary)"""
    W, H = SPECIAL_FRAME
    p, flags, pose = SPECIAL_LIGHT[k]
    case = dict(LC.random_case(W, H, ortho))
    rng = np.random.default_rng(95 + int(ortho))
    keys = case["keys"].copy()
    if pose == "down":
        case["cam"] = tuple(np.asarray(v, F32) for v in ((14.5, 44.25, 20.75),) + DOWN_POSE)
        o, d = RD.primary_rays(W, H, *case["cam"], ortho=ortho, ortho_size=case["ortho_size"])
        keys = RD.keys_np(case["hit"], case["world"].shape, o, d).copy()
    axis2 = (keys != 0) & (((keys >> np.uint32(26)) & np.uint32(31)) == 2)
    pick = rng.random((H, W))
    for i, a in enumerate(SPECIAL_AXES):
        at = axis2 & (pick >= 0.2 * i) & (pick < 0.2 * (i + 1))
        keys[at] = (keys[at] & np.uint32(0x83FFFFFF)) | np.uint32(a << 26)
    other = rng.random((H, W))
    hitk = keys != 0
    keys[hitk & (other < 0.03)] &= np.uint32(0xFE000000)
    keys[hitk & (other >= 0.03) & (other < 0.06)] |= np.uint32(0x1FFFFFF)
    keys.setflags(write=False)
    case.update(color=special_frame()[0], keys=keys, params=dict(case["params"], **SPECIAL_LIGHT_PARAMS[p]))
    out = LC.run_case(case, flags)
    for a in out[:2]:
        a.setflags(write=False)
    return (case,) + tuple(out[:3])


def _light_reach(c):
    lines = [("flag sets", len({f for _, f, _ in SPECIAL_LIGHT}), 3), ("parameter sets", len({p for p, _, _ in SPECIAL_LIGHT}), 1)]
    for ortho in (False, True):
        case = special_light(ortho, 0)[0]
        k = case["keys"]
        hit = ((k != 0) & (case["hit"] >= 0) & (case["hit"] < 64 ** 3))[..., None]
        lines += [("kinds of special colours under hit keys", _kinds(SPECIALS, case["color"], hit), len(SPECIALS) - 1),
                  ("kinds of special colours under miss keys", _kinds(SPECIALS, case["color"], ~hit), len(SPECIALS) - 1),
                  ("axis fields above 2", len(set(np.unique((k >> np.uint32(26)) & np.uint32(31)).tolist()) & set(SPECIAL_AXES)), len(SPECIAL_AXES) - 1),
                  ("keys on plane 0", int(((k != 0) & ((k & np.uint32(0x1FFFFFF)) == 0)).sum()), 50),
                  ("keys on plane 0x1FFFFFF", int(((k & np.uint32(0x1FFFFFF)) == 0x1FFFFFF).sum()), 50)]
    return lines


SPECIAL_LIGHT_CASE = Case(
    "special_light", "vxrt_light_frame.hpp: lf_shade on NaN, infinite, negative-zero and denormal colours, parameters at both ends, axis fields above 2",
    dict(frame=SPECIAL_FRAME, runs=SPECIAL_LIGHT), _light_reach)

# ---- 9. LIGHT_LARGE_WORLD: vxrt_light_frame on the bench world of tests/read_limit_cases.py (8192 x 512 x 8192, brick edge 32)
LARGE_BOX = ((-5, -5, -5), (300, 200, 300))  # a light box over the world's three low faces
LARGE_ORTHO = (40.0, 30.0)


def large_hits(W, H, seed=0):
    """tests/read_limit_cases.py's guide_hits (random indices over the world and beyond, misses, GUIDE_HITS at the first and
    the last pixels) with every fifth pixel between them on one of the world's six boundary layers or in the corner the light
    box covers: (int64 [H, W], int [H, W]: 0 .. 5 the boundary layer, 6 the corner, -1 elsewhere)"""
    hit = guide_hits(W, H, seed).reshape(-1).copy()
    rng = np.random.default_rng(97 + seed)
    dims = np.array(GUIDE_WORLD[:3], np.int64)
    at = np.arange(len(GUIDE_HITS) + 5, W * H - len(GUIDE_HITS), 5)
    v = np.stack([rng.integers(0, n, len(at)) for n in dims], -1)
    kind = rng.integers(0, 8, len(at))
    for side in range(6):
        v[kind == side, side >> 1] = dims[side >> 1] - 1 if side & 1 else 0
    v[kind >= 6] = np.stack([rng.integers(0, n - 5, int((kind >= 6).sum())) for n in LARGE_BOX[1]], -1)
    hit[at] = v[:, 0] + dims[0] * (v[:, 1] + dims[1] * v[:, 2])
    kinds = np.full(W * H, -1)
    kinds[at] = np.minimum(kind, 6)
    return hit.reshape(H, W), kinds.reshape(H, W)


@functools.lru_cache(maxsize=None)
def large_levels():
    lv = np.random.default_rng(98).integers(0, 256, LARGE_BOX[1], dtype=np.uint8)
    lv.setflags(write=False)
    return lv


def _large_total():
    return GUIDE_WORLD[0] * GUIDE_WORLD[1] * GUIDE_WORLD[2]


LIGHT_LARGE_WORLD = Case(
    "light_large_world", "vxrt_light_frame.hpp: lf_load's 64-bit decode of hit indices of 2^32 and more, lf_solid on the bench world's grid",
    dict(world=GUIDE_WORLD, frames=GUIDE_FRAMES, box=LARGE_BOX),
    lambda c: [("voxels of the world", _large_total(), 1 << 32),
               ("largest index inside the world", max(h for h in GUIDE_HITS if h < _large_total()), 1 << 32),
               ("hits of the small frame at 2^32 and more inside the world", int(((large_hits(*GUIDE_FRAMES[0])[0] >= 1 << 32) & (large_hits(*GUIDE_FRAMES[0])[0] < _large_total())).sum()), 1000),
               ("boundary layers and the corner with hits", len(set(np.unique(large_hits(*GUIDE_FRAMES[0])[1]).tolist()) - {-1}), 6),
               ("indices outside the world", sum(h >= _large_total() for h in GUIDE_HITS), 1),
               ("side", max(max(f) for f in GUIDE_FRAMES), c["dn_max_side"] - 1)])

# ---- 7. PIXEL_LIMIT: a frame four pixels short of kDnMaxPixels; inputs that are functions of the pixel index alone
LIMIT_FRAME = (8190, 8194)
LIMIT_BAND, LIMIT_MARGIN = 6, 8  # rows of a band; history rows around it given to the banded restatement
LIMIT_KEYS = (0, 0x80000005, 0x84000005, 0x8A000007, 0x82000005, 0x84000005, 0x84000005, 0x8A000007)  # by hash: one miss in eight
LIMIT_N = (0.0, 1.0, 1.0, 2.0, 3.0, 5.0, 7.0, 7.0)
LIMIT_FOREIGN = 0x88000009
LIMIT_MAX_HISTORY = 7
_M32 = 0xFFFFFFFF


def hash32(i, salt):
    """an integer hash of the int64 array or tensor i (below 2^30) to 0 .. 2^32 - 1, with operators numpy and torch share"""
    x = (i + salt * 0x9E3779B1) & _M32
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & _M32
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & _M32
    return x ^ (x >> 16)


def limit_bands():
    """the first rows of the bands: the frame's first and last rows, the rows around pixel index 2^25, two by a fixed seed"""
    W, H = LIMIT_FRAME
    rng = np.random.default_rng(99)
    return (0, H - LIMIT_BAND, (1 << 25) // W - 2) + tuple(int(v) for v in rng.integers(100, H - 100, 2))


def limit_reproject_inputs(i, table, f32):
    """(colour [n, 3], keys [n], history [n, 4], previous keys [n]) of the pixels of index i; table(values) makes a lookup
    table of the array kind of i, f32(x) converts to binary32"""
    color = f32(hash32(3 * i[:, None] + table((0, 1, 2))[None, :], 1) & 1023) / 1024
    keys = table(LIMIT_KEYS)[hash32(i, 2) & 7]
    foreign = (hash32(i, 3) % 10) == 0
    kprev = keys * (~foreign) + LIMIT_FOREIGN * foreign
    rgb = f32(hash32(3 * i[:, None] + table((0, 1, 2))[None, :], 4) & 1023) / 1024
    n = table(LIMIT_N)[hash32(i, 5) & 7]
    return color, keys, rgb, f32(n), kprev


def limit_cameras():
    """an orthonormal pose above the planes the keys name and a previous camera a thousandth of a voxel away: the taps of a
    pixel stay within a row or two of it"""
    fwd, up, right = thin_pose()
    pos = np.array([9.0, 14.0, 6.0])
    return (tuple(np.asarray(v, F32) for v in (pos, fwd, up, right)),
            tuple(np.asarray(v, F32) for v in (pos + 0.002 * right + 0.001 * up, fwd, up, right)))


def limit_reproject_band(y0):
    """the banded restatement of rows y0 .. y0 + LIMIT_BAND - 1: (records, the band's counts)"""
    from tests import ref_reproject as T
    W, H = LIMIT_FRAME
    y1 = y0 + LIMIT_BAND
    h0, h1 = max(y0 - LIMIT_MARGIN, 0), min(y1 + LIMIT_MARGIN, H)
    table = lambda v: np.asarray(v, np.float32 if isinstance(v[0], float) else np.int64)
    f32 = lambda x: x.astype(F32)
    color, keys, _, _, _ = limit_reproject_inputs(np.arange(y0 * W, y1 * W, dtype=np.int64), table, f32)
    _, _, rgb, n, kprev = limit_reproject_inputs(np.arange(h0 * W, h1 * W, dtype=np.int64), table, f32)
    cur, prev = limit_cameras()
    o, d = RD.primary_rays(W, H, *cur, rows=(y0, y1))
    hist = np.concatenate([rgb, n[:, None]], -1).reshape(h1 - h0, W, 4)
    return T.reproject_np(color.reshape(LIMIT_BAND, W, 3), keys.astype(np.uint32).reshape(LIMIT_BAND, W), o, d, prev, T.camera_constants(W, H), hist,
                          kprev.astype(np.uint32).reshape(h1 - h0, W), LIMIT_MAX_HISTORY, rows=(y0, y1), frame_h=H, hist_rows=(h0, h1))


def limit_light_inputs(i, table, f32):
    """(colour [n, 3], hit index [n]) of the pixels of index i for the light on frames in the 64^3 world: by hash a voxel
    anywhere in the world (one half), on one of its six boundary layers (a quarter), an index beyond the world, or -1"""
    color = f32(hash32(3 * i[:, None] + table((0, 1, 2))[None, :], 6) & 1023) / 1024
    kind = hash32(i, 7) & 15
    axis, far = hash32(i, 11) % 3, hash32(i, 12) & 1
    v = []
    for k in range(3):
        on_face = ((kind >= 8) & (kind < 12) & (axis == k)) * 1
        v.append((hash32(i, 8 + k) & 63) * (1 - on_face) + 63 * far * on_face)
    hit = v[0] + 64 * (v[1] + 64 * v[2])
    beyond, miss = ((kind == 12) | (kind == 13)) * 1, (kind >= 14) * 1
    hit = hit * (1 - beyond) + (64 ** 3 + (hash32(i, 13) & 3) * (1 << 40)) * beyond
    return color, hit * (1 - miss) - miss


def limit_light_band(y0):
    """the restatement of rows y0 .. y0 + LIMIT_BAND - 1 on the world, the levels, the box and the camera of
    tests/light_frame_cases.py's random case (8, 8): (the band's keys, colours, terms, counts)"""
    W, H = LIMIT_FRAME
    y1 = y0 + LIMIT_BAND
    case = LC.random_case(8, 8, False)
    table = lambda v: np.asarray(v, np.float32 if isinstance(v[0], float) else np.int64)
    color, hit = limit_light_inputs(np.arange(y0 * W, y1 * W, dtype=np.int64), table, lambda x: x.astype(F32))
    o, d = RD.primary_rays(W, H, *case["cam"], rows=(y0, y1))
    hit = hit.reshape(LIMIT_BAND, W)
    keys = RD.keys_np(hit, case["world"].shape, o, d)
    out = LF.light_frame_np(color.reshape(LIMIT_BAND, W, 3), keys, hit, o, d, case["world"], case["levels"], case["box"], case["params"])
    return (keys,) + tuple(out[:3])


PIXEL_LIMIT = Case(
    "pixel_limit", "vxrt_reproject.hpp, vxrt_light_frame.hpp: pixel indices near 2^26, 3 i + 2 near 2^28, 2^18 tiles, 129 tiles a wave",
    dict(frame=LIMIT_FRAME, bands=limit_bands()),
    lambda c: [("pixels", LIMIT_FRAME[0] * LIMIT_FRAME[1], c["dn_max_pixels"] - 5),
               ("tiles", frame_launch(*LIMIT_FRAME, False, NOMINAL_CUS, c).tiles, 1 << 18),
               ("tiles a wave of the counted launch walks", frame_launch(*LIMIT_FRAME, True, NOMINAL_CUS, c).per_wave, 127),
               ("index of the last colour", 3 * LIMIT_FRAME[0] * LIMIT_FRAME[1] - 1, 3 * c["dn_max_pixels"] - 14),
               ("bands", len(limit_bands()), 4)])

FRAME_CASES = [THIN_FRAMES_CASE, PIXEL_LIMIT, SPECIAL_REPROJECT_CASE, SPECIAL_LIGHT_CASE, LIGHT_LARGE_WORLD, LIGHT_BOX_LIMITS, LIGHT_THREE_SIDES]
LAUNCH_CASES = RULE_CASES + FRAME_CASES
