"""World-query limit cases: calls of the world queries (edits and stamps, islands, nav) whose shapes reach the code that only
runs past a launch cap.

The caps live in voxelengine_amd/csrc and include/vxrt.h; read_caps() reads them with regexes:
- k_nav_level grid-strides over one level's tile list past kNavLevelGroups workgroups (vxrt_nav.hip);
- k_nav_zpass grid-strides over B's plane words past kNavZpassGroups x 256 lanes;
- k_nav_goals runs one 256-lane workgroup per 256 goals (up to VXRT_NAV_MAX_GOALS);
- k_nav_paths grid-strides over the starts past 4096 x 256 lanes, and a path makes up to VXRT_NAV_MAX_STEPS moves;
- k_isl_output grid-strides past 65536 workgroups x 4 waves x kIslPairsPerWave pairs of region words, and flushes a
  wave's counts whenever the island changes (vxrt_islands.hip);
- k_edit_bricks / k_stamp_bricks filter up to kEditMaxOps ops with 256 lanes, start the list at the last op that covers the
  whole brick and compact it by ballot in chunks of 64 ops (vxrt_edit.hip, vxrt_region.hip).
Every case names the cap it must exceed; tests/test_query_limits_host.py asserts that it does (and that raising any cap
breaks that), so a raised cap fails there instead of leaving tests/test_gpu_query_limits.py short of its path.

Closed-form references for the cases too large for the restatements (each held against them at small sizes by the host
test): the serpentine corridor's distances and next codes from its cells in path order, the islands of a 3-D parity
checkerboard (every solid voxel its own component), and a vectorised decoding of nav paths (tests/ref_nav.decode_paths
follows one start at a time)."""
from __future__ import annotations

import os
import re

import numpy as np

from tests import ref_nav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP_SOURCES = {  # name: (file, regex whose group 1 is the value); each must match exactly once
    "nav_level_groups": ("voxelengine_amd/csrc/vxrt_nav.hip", r"constexpr uint32_t kNavLevelGroups = (\d+);"),
    "nav_zpass_groups": ("voxelengine_amd/csrc/vxrt_nav.hip", r"constexpr uint32_t kNavZpassGroups = (\d+);"),
    "nav_goal_lanes": ("voxelengine_amd/csrc/vxrt_nav.hip", r"k_nav_goals, dim3\(\(ngoals \+ \d+u\) / (\d+)u\)"),
    "nav_paths_blocks": ("voxelengine_amd/csrc/vxrt_nav.hip", r"k_nav_paths, dim3\(blocks > (\d+)u \? \1u"),
    "nav_tile_y": ("voxelengine_amd/csrc/vxrt_nav.hpp", r"constexpr int kNavTileY = (\d+), kNavTileZ = \d+;"),
    "nav_tile_z": ("voxelengine_amd/csrc/vxrt_nav.hpp", r"constexpr int kNavTileY = \d+, kNavTileZ = (\d+);"),
    "nav_max_goals": ("include/vxrt.h", r"#define VXRT_NAV_MAX_GOALS (\d+)"),
    "nav_max_steps": ("include/vxrt.h", r"#define VXRT_NAV_MAX_STEPS (\d+)"),
    "isl_output_blocks": ("voxelengine_amd/csrc/vxrt_islands.hip", r"k_isl_output, dim3\(ob > (\d+)u \? \1u"),
    "isl_pairs_per_wave": ("voxelengine_amd/csrc/vxrt_islands.hip", r"constexpr uint32_t kIslPairsPerWave = (\d+);"),
    "edit_max_ops": ("voxelengine_amd/csrc/vxrt_edit.hpp", r"constexpr uint32_t kEditMaxOps = (\d+);"),
    "edit_max_ops_h": ("include/vxrt.h", r"#define VXRT_EDIT_MAX_OPS (\d+)"),
    "edit_filter_lanes": ("voxelengine_amd/csrc/vxrt_edit.hip", r"__launch_bounds__\((\d+)\) void k_edit_bricks"),
    "edit_chunk": ("voxelengine_amd/csrc/vxrt_edit.hip", r"base < nops; base \+= (\d+)u\)"),
    "stamp_filter_lanes": ("voxelengine_amd/csrc/vxrt_region.hip", r"__launch_bounds__\((\d+)\) void k_stamp_bricks"),
    "stamp_chunk": ("voxelengine_amd/csrc/vxrt_region.hip", r"base < nst; base \+= (\d+)u\)"),
}


def read_caps(root=ROOT):
    caps = {}
    for name, (path, rx) in CAP_SOURCES.items():
        with open(os.path.join(root, path)) as f:
            found = re.findall(rx, f.read())
        assert len(found) == 1, (name, path, rx, found)
        caps[name] = int(found[0])
    return caps


def ceil_div(a, b):
    return -(-a // b)


def region_words(dims):
    return ceil_div(dims[0], 32) * dims[1] * dims[2]


def nav_tiles(dims, caps):
    """tiles_total: 32 x kNavTileY x kNavTileZ cells per tile (one region word of x per lane)"""
    return ceil_div(dims[0], 32) * ceil_div(dims[1], caps["nav_tile_y"]) * ceil_div(dims[2], caps["nav_tile_z"])


class Case:
    """a name, the path it targets (file: what), its shape, and reach(caps) -> [(what, value, bound)]: value > bound each"""

    def __init__(self, name, path, shape, reach):
        self.name, self.path, self.shape, self.reach = name, path, dict(shape), reach

    def __repr__(self):
        return "Case(%s)" % self.name


# ---- nav
NAV_WINDOW = Case(
    "nav_window_4096_goals", "vxrt_nav.hip: k_nav_level / k_nav_zpass grid-stride, k_nav_goals over 16 workgroups",
    dict(world=(8192, 512, 8192, 32), corner=(3000, 2000), dims=(1024, 64, 1024), agent=(1, 2, 1, 3), goals=4096,
         repeat_from=3072, repeat_stride=256, max_dist=12),
    lambda c: [("tiles of B", nav_tiles((1024, 64, 1024), c), c["nav_level_groups"]),
               ("plane words of B", region_words((1024, 64, 1024)), c["nav_zpass_groups"] * 256),
               ("goals", 4096, c["nav_max_goals"] - 1), ("goal workgroups", 4096 // c["nav_goal_lanes"], 1),
               ("repeat distance", 256, c["nav_goal_lanes"] - 1)])
NAV_PATHS = Case(
    "nav_paths_1m_starts", "vxrt_nav.hip: k_nav_paths grid-stride",
    dict(nodes=1 << 20, non_nodes=4096, outside=8192, max_steps=16),
    lambda c: [("starts", (1 << 20) + 4096 + 8192, c["nav_paths_blocks"] * 256)])
NAV_SNAKE = Case(
    "nav_snake_65535_steps", "vxrt_nav.hip: k_nav_paths at max_steps = VXRT_NAV_MAX_STEPS; 131k BFS levels",
    dict(X=512, Z=512, height=64, factor=8, agent=(1, 2, 1, 3)),
    lambda c: [("moves of the corridor", len(snake_path(512, 512)) - 1, c["nav_max_steps"]),
               ("distance of the truncated start", c["nav_max_steps"] + 1, c["nav_max_steps"])])

# ---- islands
ISL_THIN = Case(
    "islands_thin_box_2_24_words", "vxrt_islands.hip: k_isl_output grid-stride",
    dict(world=(64, 4096, 4096), factor=8, origin=(21, 0, 0), dims=(1, 4096, 4096), density=0.55, max_islands=1 << 21),
    lambda c: [("region words", region_words((1, 4096, 4096)), c["isl_output_blocks"] * 4 * c["isl_pairs_per_wave"] * 2)])
ISL_CHECKER = Case(
    "islands_checkerboard_256", "vxrt_islands.hip: k_isl_output's per-wave flush at every solid voxel",
    dict(dims=(256, 256, 256), factor=16, max_islands=(1 << 23, 1000)),
    lambda c: [("islands of one wave step (16 per 32-voxel word)", 32, 1)])

# ---- edits and stamps
COVER_AT = (63, 64, 255, 256, 1023)  # indices of the last op / replace stamp that covers a whole brick
EDIT_1024 = Case(
    "edit_1024_ops", "vxrt_edit.hip: k_edit_bricks' op filter (256 lanes), list start `first`, 64-op ballot chunks",
    dict(ops=1024, cover_at=COVER_AT),
    lambda c: [("ops", 1024, c["edit_max_ops"] - 1), ("last covering op", max(COVER_AT), c["edit_filter_lanes"] - 1),
               ("covering ops past the first chunk", sum(k >= c["edit_chunk"] for k in COVER_AT), 2)])
STAMP_1024 = Case(
    "stamp_1024_stamps", "vxrt_region.hip: k_stamp_bricks' stamp filter, list start `first`, 64-stamp ballot chunks",
    dict(stamps=1024, cover_at=COVER_AT),
    lambda c: [("stamps", 1024, c["edit_max_ops"] - 1), ("last covering stamp", max(COVER_AT), c["stamp_filter_lanes"] - 1),
               ("covering stamps past the first chunk", sum(k >= c["stamp_chunk"] for k in COVER_AT), 2)])

LAUNCH_CASES = [NAV_WINDOW, NAV_PATHS, NAV_SNAKE, ISL_THIN, ISL_CHECKER, EDIT_1024, STAMP_1024]


# ---- closed forms
def snake_path(X, Z):
    """the cells (x, z) of ref_nav.snake_world(X, Z)'s corridor at y = 1 in path order from (0, 0): the open rows z = 0, 2,
    .. alternately left to right and right to left, joined by the gaps of the walled rows between them (the k-th walled
    row is open at X - 1 for even k, at 0 for odd k); with Z even a last walled row ends the path at its gap"""
    cells = []
    for r, z in enumerate(range(0, Z, 2)):
        xs = range(X) if r % 2 == 0 else range(X - 1, -1, -1)
        cells += [(x, z) for x in xs]
        if z + 1 < Z:
            cells.append((X - 1 if r % 2 == 0 else 0, z + 1))
    return cells


def snake_field(X, Z, Y, agent=(1, 2, 1, 3)):
    """dist and next (uint32 / uint8 [x, y, z] over B = [0, X) x [0, Y) x [0, Z)) toward the goal (0, 1, 0) of the
    corridor, for an agent that reaches no wall top (width 1, height <= 3, climb and drop < 4: the walls are 4 high): the
    i-th cell of the path is at distance i and its next code is the move to cell i - 1, its only neighbour one level down.
    Returns (dist, next, path)"""
    assert agent[0] == 1 and agent[1] <= 3 and agent[2] < 4 and agent[3] < 4
    path = np.asarray(snake_path(X, Z), np.int64)
    dist = np.full((X, Y, Z), ref_nav.UNREACHED, np.uint32)
    nxt = np.full((X, Y, Z), ref_nav.NONE, np.uint8)
    dist[path[:, 0], 1, path[:, 1]] = np.arange(len(path), dtype=np.uint32)
    per = 1 + agent[2] + agent[3]
    step = path[:-1] - path[1:]                         # cell i -> cell i - 1
    k = np.select([step[:, 0] == 1, step[:, 0] == -1, step[:, 1] == 1], [0, 1, 2], 3)  # ref_nav.DIRS order
    nxt[path[1:, 0], 1, path[1:, 1]] = (1 + k * per).astype(np.uint8)
    nxt[0, 1, 0] = 0
    return dist, nxt, path


def checkerboard(dims, origin=(0, 0, 0)):
    """bool [x, y, z]: solid where the world coordinates sum to an even number"""
    x = np.arange(dims[0], dtype=np.int64)[:, None, None] + origin[0]
    y = np.arange(dims[1], dtype=np.int64)[None, :, None] + origin[1]
    z = np.arange(dims[2], dtype=np.int64)[None, None, :] + origin[2]
    return (x + y + z) % 2 == 0


def checker_islands(dims, origin, anchors):
    """the islands of a checkerboard box: no two solid voxels share a face, so each is its own component (id = 1 + its
    region index) and an island exactly when it is not an anchor voxel.  Returns (summary, floating, ids, lo): ids
    ascending, lo (n, 3) world voxels; every island has one voxel and hi = lo + 1"""
    from tests import ref_islands
    solid = checkerboard(dims, origin)
    isl = solid & ~ref_islands.anchor_mask(dims, origin, anchors)
    z, y, x = np.nonzero(isl.transpose(2, 1, 0))        # region order: x fastest, then y, then z
    ids = 1 + x.astype(np.int64) + dims[0] * (y.astype(np.int64) + dims[1] * z.astype(np.int64))
    lo = np.stack([x, y, z], 1).astype(np.int64) + np.asarray(origin, np.int64)
    return (int(solid.sum()), len(ids), len(ids)), isl, ids, lo


def decode_paths_np(nxt, origin, agent, starts, max_steps, cells=True):
    """ref_nav.decode_paths over all starts at once (one numpy step per move): (cells or None, lengths, status)"""
    dims = np.asarray(nxt.shape, np.int64)
    o = np.asarray(origin, np.int64)
    starts = np.asarray(starts, np.int64).reshape(-1, 3)
    n = len(starts)
    mv = np.zeros((256, 3), np.int64)
    valid = np.zeros(256, bool)
    for code, dx, dy, dz in ref_nav.moves(agent):
        mv[code], valid[code] = (dx, dy, dz), True
    inside = lambda q: ((q - o >= 0) & (q - o < dims)).all(1)
    p = starts.copy()
    lengths = np.zeros(n, np.int32)
    status = np.full(n, -1, np.int32)
    status[~inside(starts)] = ref_nav.OUTSIDE
    out = np.zeros((n, max_steps + 1, 3), np.int32) if cells else None
    if cells:
        out[:, 0] = starts
    act = np.flatnonzero(status < 0)
    for step in range(max_steps + 1):
        if len(act) == 0:
            break
        q = p[act] - o
        code = nxt[q[:, 0], q[:, 1], q[:, 2]].astype(np.int64)
        goal, bad = code == 0, (code != 0) & ~valid[code]
        status[act[goal]] = ref_nav.AT_GOAL
        status[act[bad]] = ref_nav.NO_PATH
        go = ~goal & ~bad
        if step == max_steps:
            status[act[go]] = ref_nav.TRUNCATED
            break
        a, t = act[go], p[act[go]] + mv[code[go]]
        ok = inside(t)
        status[a[~ok]] = ref_nav.NO_PATH
        a, t = a[ok], t[ok]
        p[a] = t
        lengths[a] += 1
        if cells:
            out[a, step + 1] = t
        act = a
    assert (status >= 0).all()
    if cells:
        last = np.take_along_axis(out, np.repeat(lengths.astype(np.int64)[:, None, None], 3, 2), 1)
        pad = np.arange(max_steps + 1)[None, :] > lengths[:, None]
        out = np.where(pad[:, :, None], last, out)
    return out, lengths, status
