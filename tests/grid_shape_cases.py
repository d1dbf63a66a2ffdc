"""Grid shapes at which the wave tracer (voxelengine_amd/csrc/vxrt_wave2.hpp) treats its three axes differently: the packed
step counters (rem = x | y << 11 | z << 21: 10 value bits for x and z, 9 for y), the strides of a step (1, c_row for z,
c_slice for y), the wide-grid offsets in LDS (CF_OFF_XZ = x | z << 16, CF_OFF_Y), the four disjuncts of grid_is_wide
(vxrt_device.hpp) and the time threshold that ends a walk on an ordinary grid.  Shared by tests/test_grid_shapes_host.py,
which holds every case to the side of the predicate it names and to the coverage its rays must have (on the oracle alone),
and tests/test_gpu_grid_shapes.py, which runs them on the device.

The constants live in voxelengine_amd/csrc; read_caps() reads them with regexes that must match exactly once.

Cases, in coarse cells (f = 8; O2 and W2 also at f = 32, where the brick level is the same but the world coordinates and the
world box differ):
- O1-O3: the largest ordinary grid per axis (a full field; a far-face start arms it with `dim` itself; the longest
  accumulation of tMax against the time threshold);
- O4, O5: two adjacent fields full at once; O6: the largest sum an ordinary grid can have;
- W2, W3: the smallest grids wide by the y / the z disjunct alone (W1 = 1024 x 8 x 8 is in tests/test_gpu_parity.py);
- W4: wide by the sum alone, no field beyond its cap (16.5 M cells: the one heavy case);
- W5, W6: far beyond the caps along y / z, long enough for walks that end by MAX_STEPS;
- W7-W9: the ABI's largest dimension, 65528 cells (fx - px and fz - pz within 7 of 2^16, coordinates up to 524224).

Out of scope: cy * cz near 2^24, where the inner sum of cell_index()'s two 24-bit multiply-adds is at or above 2^23.  It
needs at least 67 M cells, 1.6 GB of bounds on the host: not a test of a few seconds.

The scenes are sparse by construction (tests/sparse_world.py): random single voxels at a density that lets about half of
the rays along a long axis cross it, and a few hundred small solid boxes."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from tests import helpers
from tests import sparse_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = "voxelengine_amd/csrc/"

CAP_SOURCES = {  # name: (file, regex whose group 1 is the value); each must match exactly once
    "field_cap_xz": (_CSRC + "vxrt_device.hpp", r"#define VXRT_FIELD_CAP_XZ (\d+)u\n"),
    "field_cap_y": (_CSRC + "vxrt_device.hpp", r"#define VXRT_FIELD_CAP_Y (\d+)u\n"),
    "max_steps": (_CSRC + "vxrt_device.hpp", r"constexpr int kMaxSteps = (\d+);"),
    "max_dim": (_CSRC + "vxrt_api.hip", r"cd\[a\] % 8 != 0 \|\| cd\[a\] > (\d+)\)"),
}
# what grid_is_wide must look like for the restatement below to be the predicate of the product (matches exactly once)
PREDICATE_SOURCE = (_CSRC + "vxrt_device.hpp",
                    r"return cx > \(int\)kFieldCapXZ \|\| cz > \(int\)kFieldCapXZ \|\| cy > \(int\)kFieldCapY \|\| cx \+ cy \+ cz \+ 4 >= kMaxSteps;")


def _matches(root, path, rx):
    with open(os.path.join(root, path)) as f:
        return re.findall(rx, f.read())


def read_caps(root=ROOT):
    caps = {}
    for name, (path, rx) in CAP_SOURCES.items():
        found = _matches(root, path, rx)
        assert len(found) == 1, (name, path, rx, found)
        caps[name] = int(found[0])
    assert len(_matches(root, *PREDICATE_SOURCE)) == 1, PREDICATE_SOURCE
    return caps


def wide_disjuncts(cells, caps):
    """grid_is_wide (vxrt_device.hpp) restated: the names of the disjuncts that hold for a grid of `cells`, () = ordinary"""
    cx, cy, cz = cells
    held = []
    if cx > caps["field_cap_xz"]:
        held.append("x")
    if cz > caps["field_cap_xz"]:
        held.append("z")
    if cy > caps["field_cap_y"]:
        held.append("y")
    if cx + cy + cz + 4 >= caps["max_steps"]:
        held.append("sum")
    return tuple(held)


def admitted(cells, caps):
    """check_shape (vxrt_api.hip) restated: positive multiples of 8 up to the limit, 32-bit cell indices"""
    cx, cy, cz = cells
    ok = all(0 < c <= caps["max_dim"] and c % 8 == 0 for c in cells)
    return ok and cy * cz < 1 << 24 and cx * cz * (cy + 2) + 64 < 1 << 32


class Case:
    """name; cells per axis; brick edge; the side of grid_is_wide it must be on ("ordinary" / "wide"); for a wide case the
    disjunct it reaches and whether through that one alone; what it is there for"""

    def __init__(self, name, cells, side, disjunct=None, alone=False, why="", factor=8, largest_dim=False):
        self.name, self.cells, self.factor, self.side, self.disjunct, self.alone, self.why = name, tuple(cells), factor, side, disjunct, alone, why
        self.largest_dim = largest_dim     # its longest axis is the largest dimension the ABI admits
        self.dims = tuple(c * factor for c in cells)
        self.ncells = cells[0] * cells[1] * cells[2]
        self.long_axes = tuple(a for a in range(3) if cells[a] > 4 * min(cells))
        self.seed = sum(c * k for c, k in zip(cells, (1, 3, 7))) + factor

    def __repr__(self):
        return "Case(%s)" % self.name


CASES = [
    Case("O1", (1016, 8, 8), "ordinary", why="the x field full"),
    Case("O2", (8, 504, 8), "ordinary", why="the y field (9 value bits) full; the c_slice stride"),
    Case("O3", (8, 8, 1016), "ordinary", why="the z field full, next to the guard in the sign bit"),
    Case("O4", (1016, 504, 8), "ordinary", why="the x and y fields full at once: a borrow across the field boundary"),
    Case("O5", (8, 504, 1016), "ordinary", why="the y and z fields full at once"),
    Case("O6", (1016, 8, 1016), "ordinary", why="the largest sum an ordinary grid can have"),
    Case("W2", (8, 512, 8), "wide", "y", True, "the smallest grid wide by the y disjunct alone: CF_OFF_Y"),
    Case("W3", (8, 8, 1024), "wide", "z", True, "the smallest grid wide by the z disjunct alone: the high half of CF_OFF_XZ"),
    Case("W4", (1016, 16, 1016), "wide", "sum", True, "wide by the sum alone, no field beyond its cap"),
    Case("W5", (8, 4096, 8), "wide", "y", False, "CF_OFF_Y re-armed many times; walks along y that end by MAX_STEPS"),
    Case("W6", (8, 8, 8192), "wide", "z", False, "the high half of CF_OFF_XZ re-armed many times; walks along z that end by MAX_STEPS"),
    Case("W7", (65528, 8, 8), "wide", "x", False, "the ABI's largest dimension along x", largest_dim=True),
    Case("W8", (8, 65528, 8), "wide", "y", False, "the ABI's largest dimension along y", largest_dim=True),
    Case("W9", (8, 8, 65528), "wide", "z", False, "the ABI's largest dimension along z", largest_dim=True),
    Case("O2_f32", (8, 504, 8), "ordinary", why="O2 with world coordinates up to 16128", factor=32),
    Case("W2_f32", (8, 512, 8), "wide", "y", True, "W2 with world coordinates up to 16384", factor=32),
]
BY_NAME = {c.name: c for c in CASES}
HEAVY = "W4"   # 16.5 M cells


def check_case(case, caps):
    """the reasons (strings) why `case` is not where it says it is under `caps`; [] = it is"""
    held = wide_disjuncts(case.cells, caps)
    why = []
    if not admitted(case.cells, caps):
        why.append("%s: not admitted by check_shape" % case.name)
    if case.side == "ordinary":
        if held:
            why.append("%s: must be ordinary, is wide by %s" % (case.name, held))
        # ... and the largest ordinary one along its long axes: 8 cells more along any of them make it wide
        for a in case.long_axes:
            more = list(case.cells)
            more[a] += 8
            if not wide_disjuncts(more, caps):
                why.append("%s: %s is ordinary too" % (case.name, tuple(more)))
    else:
        if case.disjunct not in held:
            why.append("%s: must be wide by %s, holds %s" % (case.name, case.disjunct, held))
        if case.alone and held != (case.disjunct,):
            why.append("%s: must be wide by %s alone, holds %s" % (case.name, case.disjunct, held))
        if case.alone:   # ... and the smallest such grid: 8 cells fewer along its long axes make it ordinary
            less = list(case.cells)
            for a in (case.long_axes if case.disjunct != "sum" else (1,)):
                less[a] -= 8
            if wide_disjuncts(less, caps):
                why.append("%s: %s is wide too" % (case.name, tuple(less)))
    if case.largest_dim and max(case.cells) != caps["max_dim"] // 8 * 8:
        why.append("%s: %d is not the largest dimension admitted (%d)" % (case.name, max(case.cells), caps["max_dim"] // 8 * 8))
    return why


# ---- scenes ---------------------------------------------------------------------------------------------------------------
N_BOXES = 300
VIEW_BOXES = 40


def density(case):
    """solid voxels per voxel: a ray along the longest axis meets 0.5 of them on the part of it one walk can cover"""
    return 0.5 / (case.factor * min(max(case.cells), 2048))


def scene_voxels(case):
    """the scene's solid voxels, (n, 3) int64: random single voxels and N_BOXES solid boxes of 2 to 6 voxels per edge"""
    rng = np.random.default_rng(case.seed)
    dims = np.array(case.dims, np.int64)
    n = int(float(np.prod(dims.astype(np.float64))) * density(case))
    single = (rng.random((n, 3)) * dims).astype(np.int64)
    size = rng.integers(2, 7, size=(N_BOXES, 3))
    lo = (rng.random((N_BOXES, 3)) * (dims - size)).astype(np.int64)
    for k in range(8):   # the first eight one voxel inside the grid's corners (the region read of the GPU test straddles one)
        far = np.array([k & 1, (k >> 1) & 1, k >> 2], bool)
        lo[k] = np.where(far, dims - size[k] - 1, 1)
    k = 8
    for a in case.long_axes:   # VIEW_BOXES in front of the cameras of views() at both ends of every long axis
        for end in (0, 1):
            sel = slice(k, k + VIEW_BOXES)
            along = rng.integers(60, 600, VIEW_BOXES)
            lo[sel] = np.clip(dims // 2 + rng.integers(-30, 27, size=(VIEW_BOXES, 3)), 0, dims - size[sel])
            lo[sel, a] = dims[a] - along - size[sel, a] if end else along
            k += VIEW_BOXES
    assert k < N_BOXES
    return np.concatenate([single, sparse_world.voxels_of_boxes(lo, size)])


@functools.lru_cache(maxsize=1)
def tables(name):
    """(coarse_bits, brick_slot, bounds, pool) of a case's scene; one case at a time is kept"""
    case = BY_NAME[name]
    t = sparse_world.tables_from_voxels(scene_voxels(case), case.cells, case.factor)
    for a in t:
        a.setflags(write=False)
    return t


def world(vxo, case):
    return vxo.World.wrap(case.factor, case.cells, *tables(case.name))


# ---- rays -----------------------------------------------------------------------------------------------------------------
NEAR_AXIS = 0.002      # the other two components of a ray "nearly along" an axis, times a standard normal
FAMILIES = ("inside", "outside", "far_face", "parallel")


def ray_groups(case):
    """the families aimed at the case's long axes: (family, axis, sign) for every long axis, both directions; for two long
    axes ("diagonal", (a, b), (sa, sb)) from corner to corner"""
    g = [(fam, a, s) for a in case.long_axes for s in (1, -1) for fam in FAMILIES]
    if len(case.long_axes) == 2:
        g += [("diagonal", case.long_axes, (sa, sb)) for sa in (1, -1) for sb in (1, -1)]
    return g


def rays(case, n, seed):
    """helpers.mixed_rays with every second ray overwritten by the families of ray_groups(case), in turn.  Returns
    (origins, directions, group) -- group[i] = the index into ray_groups(case) of ray i, -1 for a ray of mixed_rays."""
    o, d = helpers.mixed_rays(case.dims, n, seed)
    rng = np.random.default_rng(seed + 7919)
    dims = np.array(case.dims, np.float64)
    groups = ray_groups(case)
    group = np.full(n, -1, np.int64)
    slots = np.arange(0, n, 2)
    group[slots] = (slots // 2) % len(groups)
    reach = 1800 * case.factor      # voxels a walk covers well before MAX_STEPS
    for gi, (fam, ax, sg) in enumerate(groups):
        idx = np.flatnonzero(group == gi)
        m = len(idx)
        oo = rng.random((m, 3)) * dims
        dd = rng.normal(size=(m, 3)) * NEAR_AXIS
        if fam == "diagonal":
            mid = 0.25 + 0.5 * rng.random((m, 3))
            oo = mid * dims
            jitter = np.where(np.arange(m) % 2 == 0, 0.0, 1.0)    # every second one from up to a cell inside the corner
            for a, s in zip(ax, sg):
                off = jitter * rng.random(m) * case.factor
                oo[:, a] = off if s > 0 else dims[a] - off
                dd[:, a] = s * dims[a]
            other = [a for a in range(3) if a not in ax][0]
            dd[:, other] *= dims[ax[0]]
        else:
            dd[:, ax] = sg
            cross = [a for a in range(3) if a != ax]
            if fam == "inside":
                if case.cells[ax] >= 2048:   # half of them within a walk's reach of the face they are heading for
                    near = np.arange(m) % 2 == 0
                    u = rng.random(m) * reach
                    oo[near, ax] = (dims[ax] - u if sg > 0 else u)[near]
            elif fam == "outside":
                oo[:, cross] = (0.25 + 0.5 * rng.random((m, 2))) * dims[cross]
                oo[:, ax] = -3.0 if sg > 0 else dims[ax] + 3.0
            elif fam == "far_face":
                oo[:, cross] = (0.25 + 0.5 * rng.random((m, 2))) * dims[cross]
                oo[:, ax] = 0.0 if sg > 0 else dims[ax]
            else:   # exactly axis-parallel on integer cross coordinates
                dd[:, cross] = 0.0
                oo[:, cross] = np.floor(oo[:, cross])
        o[idx] = oo.astype(np.float32)
        d[idx] = dd.astype(np.float32)
    return o, d, group


def exit_face(case, o, d):
    """per ray, in binary64: (axis, sign) of the face of the grid's box through which its line leaves"""
    o, d = o.astype(np.float64), d.astype(np.float64)
    dims = np.array(case.dims, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d != 0, (np.where(d > 0, dims, 0.0) - o) / d, np.inf)
    axis = np.argmin(t, axis=1)
    return axis, np.sign(d[np.arange(len(d)), axis]).astype(np.int64)


def coverage(case, o, d, group, res):
    """what the coverage conditions count, from the oracle's results `res` (World.trace_batch) alone"""
    steps, hit = res["steps"].astype(np.int64), res["hit"] != 0
    groups = ray_groups(case)
    out = {"hits_after_400": int((hit & (steps > 400)).sum()),
           "exhausted": int((~hit & (steps >= 2048)).sum())}
    far = np.zeros(len(o), bool)
    for a in case.long_axes:
        far |= (o[:, a] == np.float32(case.dims[a])) & (d[:, a] < 0)
    out["far_face_hits"] = int((far & hit).sum())
    ax, sg = exit_face(case, o, d)
    left = ~hit & (steps > 0) & (steps < 2048)
    for a in case.long_axes:
        want = min(0.9 * case.cells[a], 2047)
        for s in (1, -1):
            along = np.isin(group, [gi for gi, g in enumerate(groups) if g[0] != "diagonal" and g[1] == a and g[2] == s])
            out["long_walks", a, s] = int((along & (steps >= want)).sum())
            out["left_through", a, s] = int((left & (ax == a) & (sg == s)).sum())
    return out


def coverage_shortfalls(case, cov):
    """the coverage conditions `cov` misses, as strings; [] = all hold"""
    bad = []
    for a in case.long_axes:
        for s in (1, -1):
            if cov["long_walks", a, s] < 100:
                bad.append("walks of 0.9 x the cells along axis %d, direction %+d: %d" % (a, s, cov["long_walks", a, s]))
            if cov["left_through", a, s] < 100:
                bad.append("misses leaving through the far face of axis %d, direction %+d: %d" % (a, s, cov["left_through", a, s]))
    if max(case.cells) >= 2048 and cov["exhausted"] < 100:
        bad.append("walks that end by MAX_STEPS: %d" % cov["exhausted"])
    if cov["hits_after_400"] < 100:
        bad.append("hits after more than 400 steps: %d" % cov["hits_after_400"])
    if cov["far_face_hits"] < 50:
        bad.append("far-face starts that hit: %d" % cov["far_face_hits"])
    return bad


N_RAYS = 40000


# ---- views ----------------------------------------------------------------------------------------------------------------
FRAME_W, FRAME_H, FRAME_NUMBER = 96, 64, 3
VIEW_FOV = 30.0


def _look(fwd, hint):
    f = np.asarray(fwd, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(np.asarray(hint, np.float64), f)
    r = r / np.linalg.norm(r)
    return tuple(tuple(float(np.float32(c)) for c in v) for v in (f, np.cross(f, r), r))


def views(case):
    """the frames of a case, per long axis a: `along`, a perspective camera 20 voxels from the near end looking up the
    axis, 3 degrees off it; `light`, the same with light_dir nearly along the axis (shadow rays from the side faces of
    what it sees walk to the far end); `ortho`, an exactly axis-aligned orthographic view down the axis from its far end
    (every lane special); for y also `shaft`, a perspective camera looking straight down the axis.  Each is
    dict(name, cam = (origin, fwd, up, right), kw = keywords of vxo.make_params)."""
    out = []
    dims = np.array(case.dims, np.float64)
    unit = np.eye(3)
    for a in case.long_axes:
        b, c = [k for k in range(3) if k != a]
        pos = dims / 2 + 0.37
        pos[a] = 20.5
        cam = (tuple(float(v) for v in pos),) + _look(unit[a] + 0.05 * unit[b] + 0.03 * unit[c], unit[b])
        light = unit[a] + 0.02 * unit[b] + 0.01 * unit[c]
        out.append(dict(name="along_%d" % a, cam=cam, kw=dict(fov=VIEW_FOV)))
        out.append(dict(name="light_%d" % a, cam=cam, kw=dict(fov=VIEW_FOV, light_dir=tuple(float(np.float32(v)) for v in light / np.linalg.norm(light)))))
        far = dims / 2 + 0.25
        far[a] = dims[a] - 20.5
        axis_cam = (tuple(float(v) for v in far), tuple(float(v) for v in -unit[a]), tuple(float(v) for v in unit[b]), tuple(float(v) for v in unit[c]))
        out.append(dict(name="ortho_%d" % a, cam=axis_cam, kw=dict(ortho=1, ortho_size=(48.0, 48.0))))
        if a == 1:
            out.append(dict(name="shaft_%d" % a, cam=axis_cam, kw=dict(fov=VIEW_FOV)))
    return out
