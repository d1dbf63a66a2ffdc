"""CPU checks of the voxel materials (include/vxrt.h, vxrt_material_field / vxrt_material_frame): the two restatements of
tests/ref_material.py against each other on the cases of tests/material_cases.py, what those cases exercise (checked on the
restatement alone, so that a case set cannot hide a branch), hand-derived scenes with the expected bytes and colours written
out, the kernels' per-lane and per-pixel code (csrc/vxrt_material.hpp) compiled for the host (tests/tools/material_check.cpp)
against the restatement -- bytes, colours, BGRA8, ids and summaries bit-equal, every index checked, at several task cuts --
and the limits and the order of the refusals (tests/tools/material_args_check.cpp)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import material_cases as MC
from tests import ref_denoise as R
from tests import ref_light_frame as LF
from tests import ref_material as M
from tests.helpers import build_harness, run_harness, run_harness_files

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _field(i, paint=True, rules=MC.RULES):
    origin, dims = MC.FIELD_BOXES[i]
    out = M.material_field_np(MC.terrain_world(), origin, dims, rules, MC.paint_bytes() if paint else None, MC.PAINT_BOX)
    out[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _frame(W, H, ortho, pose, **kw):
    out = MC.run_frame(MC.frame_case(W, H, ortho, pose), **kw)
    for a in out[:2]:
        a.setflags(write=False)
    return out


# ---- the restatements against each other -------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(MC.FIELD_BOXES)))
def test_the_field_restatements_agree(i):
    origin, dims = MC.FIELD_BOXES[i]
    if dims[0] * dims[1] * dims[2] > 70000:  # the scalar loop on a slab of the large boxes
        dims = (dims[0], dims[1], 2)
        a = M.material_field_np(MC.terrain_world(), origin, dims, MC.RULES, MC.paint_bytes(), MC.PAINT_BOX)
    else:
        a = _field(i)
    b = M.material_field_scalar(MC.terrain_world(), origin, dims, MC.RULES, MC.paint_bytes(), MC.PAINT_BOX)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    solid, painted, top, hist = a[1]
    assert sum(hist) == dims[0] * dims[1] * dims[2] and hist[0] == sum(hist) - solid and painted <= solid and top <= solid
    print("material field", origin, dims, "solid, painted, top", a[1][:3])


@pytest.mark.parametrize("W,H,ortho,pose", MC.FRAME_CASES)
def test_the_frame_restatements_agree(W, H, ortho, pose):
    case = MC.frame_case(W, H, ortho, pose)
    for kw in (dict(), dict(with_atlas=False, paint=False), dict(shift=0, n_tiles=1), dict(shift=6, n_tiles=3, told_tiles=2)):
        a = _frame(W, H, ortho, pose, **kw)
        b = MC.run_frame(case, scalar=True, **kw)
        assert np.array_equal(R.bits(a[0]), R.bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2], (W, H, ortho, pose, kw)
        miss = ~a[3]["hit"]
        assert np.array_equal(R.bits(a[0][miss]), R.bits(case["color"][miss])) and not a[1][miss].any()
    # the position on the face is ref_light_frame.py's: the same pixels clamped low, and the same at the centre
    lf = LF.light_frame_np(case["color"], case["keys"], case["hit"], case["o"], case["d"], case["world"], None, ((0, 0, 0), (1, 1, 1)))[3]
    info = _frame(W, H, ortho, pose)[3]
    assert np.array_equal(lf["hit"], info["hit"]) and np.array_equal(lf["centre"], info["centre"])
    assert np.array_equal(lf["low"], info["low"]) and np.array_equal(lf["high"], info["clamped_high"])
    print("material frame", W, H, ortho, pose, "hit, painted, top, textured", _frame(W, H, ortho, pose)[2])


def test_the_cases_reach_every_branch():
    """on the restatement alone, over the case sets.  Field: every band with each of top / under / deep, under_depth 0 and 15
    deciding (a run of exactly 15 is `under`, one of 16 or more `deep`), painted and ruled voxels, paint 0 inside P, solid
    voxels outside P, a band edge inside a box.  Frame: every face class on every axis it can occur on, both texture
    fallbacks (no atlas, a tile at or beyond n_tiles) and the last tile, painted and ruled pixels, hits inside and outside P,
    iu and iw at 0 and at T - 1 -- through the clamp too --, the centre fallback, miss pixels."""
    world, run = MC.terrain_world(), M.runs_of(MC.terrain_world())
    seen = set()
    for i in range(len(MC.FIELD_BOXES)):
        seen |= set(np.unique(_field(i, paint=False)[0]).tolist())
        origin, dims = MC.FIELD_BOXES[i]
        assert any(origin[1] < e < origin[1] + dims[1] for e in (20, 32, 50))
    assert seen >= set(range(0, 13)) - {5}, seen  # band 1 has under_depth 0: its `under` (5) never decides
    assert 5 not in seen
    ys = np.arange(64)[None, :, None]
    band2 = world & (ys >= 32) & (ys < 50)
    assert (band2 & (run == 15)).any() and (band2 & (run >= 16)).any() and (band2 & (run == 1)).any()
    whole = _field(5)
    assert whole[1][1] > 0 and whole[1][1] < whole[1][0]
    po, pd = MC.PAINT_BOX
    inside = np.zeros(MC.WORLD, bool)
    inside[max(po[0], 0):po[0] + pd[0], po[1]:po[1] + pd[1], po[2]:po[2] + pd[2]] = True
    painted = whole[0] >= 100
    assert (world & inside & ~painted).any() and (world & ~inside).any() and not (painted & ~inside).any()

    faces, flags = set(), dict(no_tile=0, last_tile=0, painted=0, ruled=0, in_p=0, out_p=0, centre=0, miss=0, i0=0, iT=0, clamp_hi=0, clamp_lo=0)
    for W, H, ortho, pose in MC.FRAME_CASES:
        out, aov, summary, info = _frame(W, H, ortho, pose)
        hit = info["hit"]
        faces |= set(zip(info["a"][hit].tolist(), info["toward"][hit].tolist(), info["cls"][hit].tolist()))
        flags["no_tile"] += int((hit & ~info["textured"]).sum())
        flags["last_tile"] += int((hit & (info["tile"] == 4)).sum())
        flags["painted"] += int((hit & info["painted"]).sum())
        flags["ruled"] += int((hit & ~info["painted"]).sum())
        flags["in_p"] += int((hit & info["in_paint_box"] & ~info["painted"]).sum())
        flags["out_p"] += int((hit & ~info["in_paint_box"]).sum())
        flags["centre"] += int((hit & info["centre"]).sum())
        flags["miss"] += int((~hit).sum())
        proper = hit & ~info["centre"]
        flags["i0"] += int((proper & (info["iu"] == 0) & (info["iw"] == 0)).sum())
        flags["iT"] += int((proper & (info["iu"] == 7) & (info["iw"] == 7)).sum())
        flags["clamp_hi"] += int((proper & info["clamped_high"] & ((info["iu"] == 7) | (info["iw"] == 7))).sum())
        flags["clamp_lo"] += int((proper & info["low"]).sum())
        bare = _frame(W, H, ortho, pose, with_atlas=False, paint=False)
        assert bare[2][3] == 0 and bare[2][1] == 0 and (W * H < 100 or not np.array_equal(R.bits(bare[0]), R.bits(out)))
        if pose == "zero":
            assert (info["centre"] | ~hit).all() and hit.sum() > 10
    print("material frame branches", sorted(faces), flags)
    # (axis, toward, class): top = 0, side = 1, bottom = 2
    assert faces == {(0, 0, 1), (0, 1, 1), (1, 0, 0), (1, 1, 2), (2, 0, 1), (2, 1, 1)}
    assert all(v > 0 for v in flags.values()), flags


# ---- hand-derived scenes -----------------------------------------------------------------------------------------------
THREE = ((None, 1, 2, 3, 2),)  # grass on top, two of dirt, stone below


def test_a_three_layer_column():
    """a column x = z = 4 of y = 3 .. 9 under THREE: y = 9 has nothing above (1), y = 8 and 7 have one and two above (2), the
    rest three or more (3)"""
    w = np.zeros(MC.WORLD, bool)
    w[4, 3:10, 4] = True
    for fn in (M.material_field_np, M.material_field_scalar):
        out, (solid, painted, top, hist) = fn(w, (4, 0, 4), (1, 12, 1), THREE)
        assert out[0, :, 0].tolist() == [0, 0, 0, 3, 3, 3, 3, 2, 2, 1, 0, 0]
        assert (solid, painted, top) == (7, 0, 1) and hist[:4] == [5, 1, 2, 4] and sum(hist) == 12


def test_an_overhang():
    """a floor y = 0 .. 5 and a slab y = 10 .. 11 over it, in one band with under_depth 2: the slab's top y = 11 is `top`, its
    underside y = 10 has one above: `under`; the floor's top y = 5 has air above it -- `top` again, whatever hangs higher --
    then 4 and 3 `under`, 2 .. 0 `deep`.  With under_depth 0 the underside is `deep`."""
    w = np.zeros(MC.WORLD, bool)
    w[4, 0:6, 4] = True
    w[4, 10:12, 4] = True
    for fn in (M.material_field_np, M.material_field_scalar):
        out, (solid, painted, top, hist) = fn(w, (4, 0, 4), (1, 13, 1), THREE)
        assert out[0, :, 0].tolist() == [3, 3, 3, 2, 2, 1, 0, 0, 0, 0, 2, 1, 0] and (solid, top) == (8, 2)
        out, _ = fn(w, (4, 0, 4), (1, 13, 1), ((None, 1, 2, 3, 0),))
        assert out[0, :, 0].tolist() == [3, 3, 3, 3, 3, 1, 0, 0, 0, 0, 3, 1, 0]


def test_a_column_that_reaches_the_worlds_top_and_the_bands():
    """a column over the whole height 0 .. 63: the voxel at y = 63 has the world's end above it -- empty: `top` of its band.
    Bands from y = 60 (ids 7, 8, 9, under_depth 15) and below (1, 2, 3, depth 2): y = 63 is 7, y = 62 .. 60 have runs 1 .. 3:
    8; y = 59 has run 4 and belongs to the lower band, whose depth is 2: 3"""
    w = np.zeros(MC.WORLD, bool)
    w[4, :, 4] = True
    rules = ((None, 1, 2, 3, 2), (60, 7, 8, 9, 15))
    for fn in (M.material_field_np, M.material_field_scalar):
        out, (solid, painted, top, hist) = fn(w, (4, 40, 4), (1, 30, 1), rules)
        assert out[0, :, 0].tolist() == [3] * 20 + [8, 8, 8, 7] + [0] * 6 and (solid, top) == (24, 1)
        # under_depth 15 in a band of its own: runs 1 .. 15 are `under`, the 16th voxel down is `deep`
        out, _ = fn(w, (4, 40, 4), (1, 24, 1), ((None, 7, 8, 9, 15),))
        assert out[0, :, 0].tolist() == [9] * 8 + [8] * 15 + [7]


def test_a_paint_byte_0_inside_the_paint_box():
    """paint over (4, 7 .. 9, 4) with bytes (50, 0, 60) from y = 7: y = 7 and 9 take the paint, y = 8 -- byte 0 -- its rule"""
    w = np.zeros(MC.WORLD, bool)
    w[4, 3:10, 4] = True
    paint = np.array([50, 0, 60], np.uint8).reshape(1, 3, 1)
    for fn in (M.material_field_np, M.material_field_scalar):
        out, (solid, painted, top, hist) = fn(w, (4, 0, 4), (1, 12, 1), THREE, paint, ((4, 7, 4), (1, 3, 1)))
        assert out[0, :, 0].tolist() == [0, 0, 0, 3, 3, 3, 3, 50, 2, 60, 0, 0]
        assert (solid, painted, top) == (7, 2, 1) and hist[50] == hist[60] == 1  # (top counts the geometry: y = 9 is painted and on top)


GRASS = {1: (0.5, 1.0, 0.25)}
TILES3 = np.zeros((3, 1, 1, 4), np.uint8)
TILES3[0, 0, 0] = (255, 255, 255, 255)   # top: white
TILES3[1, 0, 0] = (51, 102, 204, 7)      # side: 0.2, 0.4, 0.8
TILES3[2, 0, 0] = (0, 255, 0, 0)         # bottom


def test_a_grass_block_from_above_from_the_side_and_from_below():
    """one voxel (4, 20, 4) of material 1 (a single band, top = 1), tint (0.5, 1, 0.25), tiles top 0, side 1, bottom 2 of 1 x 1
    texels, colour 0.5: from above 0.5 * (tint * 1); from the side 0.5 * (tint * (0.2, 0.4, 0.8)); from below 0.5 * (tint *
    (0, 1, 0)).  Every pixel that hits is `top` (nothing above the block) and textured."""
    w = np.zeros(MC.WORLD, bool)
    w[4, 20, 4] = True
    pal = MC.plain_palette(GRASS, {1: (0, 1, 2)})
    tint = np.array(GRASS[1], F32)
    want = {"down": tint * F32(1), "upward": tint * (np.array([0, 255, 0], F32) / F32(255)),
            "+x": tint * (np.array([51, 102, 204], F32) / F32(255))}
    want["-x"] = want["+z"] = want["-z"] = want["+x"]
    pos = {"down": (4.5, 40.0, 4.5), "upward": (4.5, 2.0, 4.5), "+x": (-10.0, 20.5, 4.5), "-x": (30.0, 20.5, 4.5), "+z": (4.5, 20.5, -10.0),
           "-z": (4.5, 20.5, 30.0)}
    for name in MC.VIEWS:
        out, ids, summary, info, o = MC.view(w, name, pos[name], THREE, pal, TILES3)
        assert summary == (1, 0, 1, 1), name
        (y, x), = np.argwhere(ids == 1)
        assert np.array_equal(out[y, x], F32(0.5) * want[name].astype(F32)), name
        assert (np.delete(out.reshape(-1, 3), y * 8 + x, 0) == 0.5).all()
    assert want["down"].tolist() == [0.5, 1.0, 0.25] and want["upward"].tolist() == [0.0, 1.0, 0.0]
    # without an atlas, and with the tiles beyond n_tiles: the tint alone
    for atl, tiles in ((None, (0, 1, 2)), (TILES3, (3, 4, M.NO_TILE))):
        out, ids, summary, _, _ = MC.view(w, "+x", pos["+x"], THREE, MC.plain_palette(GRASS, {1: tiles}), atl)
        assert summary == (1, 0, 1, 0) and np.array_equal(out[ids == 1][0], F32(0.5) * tint)


QUAD = np.zeros((1, 2, 2, 4), np.uint8)  # rows top-down: (row 0: red, green), (row 1: blue, yellow)
QUAD[0, 0, 0], QUAD[0, 0, 1], QUAD[0, 1, 0], QUAD[0, 1, 1] = (255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255), (255, 255, 0, 255)
RED, GREEN, BLUE, YELLOW = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0)


def test_the_texel_orientation_on_each_of_the_six_faces():
    """one voxel (4, 20, 4), a 2 x 2 tile, two pixels per voxel: each face shows four texels.  By the header: on a top or
    bottom face the column follows x and the row z; on an x face the column follows z and the rows run down as y rises; on
    a z face the column follows x and the rows run down as y rises.  Written out by the half of the voxel a pixel looks at
    (low = 0, high = 1) on the two axes of the face:"""
    w = np.zeros(MC.WORLD, bool)
    w[4, 20, 4] = True
    pal = MC.plain_palette(None, {1: (0, 0, 0)})
    # {view: (the face's axes (p, q), {(half on p, half on q): colour})}
    ydown = {(0, 0): BLUE, (1, 0): YELLOW, (0, 1): RED, (1, 1): GREEN}       # (x or z half, y half): y low is the bottom row
    xface = {(0, 0): BLUE, (1, 0): RED, (0, 1): YELLOW, (1, 1): GREEN}       # (y half, z half): s follows z, r = 1 - y half
    flat = {(0, 0): RED, (1, 0): GREEN, (0, 1): BLUE, (1, 1): YELLOW}        # (x half, z half): s = x half, r = z half
    expect = {"down": ((0, 2), flat), "upward": ((0, 2), flat), "+x": ((1, 2), xface), "-x": ((1, 2), xface), "+z": ((0, 1), ydown),
              "-z": ((0, 1), ydown)}
    q = 0.25  # the rays pass the quarter points of the voxels
    pos = {"down": (4 + q, 40.0, 4 + q), "upward": (4 + q, 2.0, 4 + q), "+x": (-10.0, 20 + q, 4 + q), "-x": (30.0, 20 + q, 4 + q),
           "+z": (4 + q, 20 + q, -10.0), "-z": (4 + q, 20 + q, 30.0)}
    for name, ((p, qx), colours) in expect.items():
        out, ids, summary, info, o = MC.view(w, name, pos[name], THREE, pal, QUAD, N=16, k=2, color=1.0)
        assert summary == (4, 0, 4, 4), (name, summary)
        got = {}
        for y, x in np.argwhere(ids == 1):
            half = (int(o[y, x, p] - np.floor(o[y, x, p]) >= 0.5), int(o[y, x, qx] - np.floor(o[y, x, qx]) >= 0.5))
            got[half] = tuple(out[y, x].tolist())
        assert got == colours, (name, got)


# ---- the kernels' code on the host -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "material_check")


def _bands(rules):
    return np.array([[-(1 << 31) if r[0] is None else r[0], *r[1:]] for r in rules], np.int32)


def _region(a):
    return np.ascontiguousarray(a.transpose(2, 1, 0))  # [x, y, z] -> region order


def _run_field(exe, tmp_path, world, origin, dims, rules, paint=None, paint_box=((0, 0, 0), (1, 1, 1)), seg=64, mis=0, factor=8):
    from oracle import vxo
    header = [0, factor, *world.shape, *origin, *dims, seg, int(paint is not None), *paint_box[0], *paint_box[1], mis, len(rules), 0, 0, 0]
    arrays = [_bands(rules), vxo.dense_from_voxels(world)] + ([_region(paint)] if paint is not None else [])
    raw, stdout = run_harness_files(exe, tmp_path, header, *arrays)
    n = dims[0] * dims[1] * dims[2]
    assert raw.size == n + 1040 and int(stdout.split()[0]) >= n // 4  # (a dword store is one check for four bytes)
    s = raw[n:].view(np.uint32)
    return raw[:n].reshape(dims[::-1]).transpose(2, 1, 0), (int(s[0]), int(s[1]), int(s[2]), [int(v) for v in s[4:260]])


def _run_frame(exe, tmp_path, case, rules=MC.RULES, shift=3, n_tiles=5, with_atlas=True, paint=True, told_tiles=None, fb=True, aov=True,
               summary=True, alias=False, cus=256, factor=8, pal=None, atl=None):
    from oracle import vxo
    H, W = case["keys"].shape
    n = W * H
    if atl is None and with_atlas:
        atl = MC.atlas(n_tiles, shift)
    tints, tiles = pal or MC.palette(n_tiles)
    entries = np.zeros((256, 5), np.uint32)
    entries[:, :3] = np.ascontiguousarray(tints, F32).view(np.uint32)
    entries[:, 3] = np.asarray(tiles)[:, 0].astype(np.uint32) | np.asarray(tiles)[:, 1].astype(np.uint32) << 16
    entries[:, 4] = np.asarray(tiles)[:, 2].astype(np.uint32)
    io = int(paint) | 2 * fb | 4 * aov | 8 * summary | 16 * alias | 32 * (atl is not None)
    told = (0 if atl is None else atl.shape[0]) if told_tiles is None else told_tiles
    tshift = shift if atl is None else atl.shape[1].bit_length() - 1
    header = [1, factor, *case["world"].shape, W, H, io, cus, told, tshift, 0 if atl is None else atl.shape[0], 0, *MC.PAINT_BOX[0], *MC.PAINT_BOX[1],
              0, len(rules), 0, 0, 0]
    arrays = [_bands(rules), vxo.dense_from_voxels(case["world"]), case["color"], case["keys"], case["hit"], case["o"], case["d"], entries]
    if atl is not None:
        arrays.append(atl)
    if paint:
        arrays.append(_region(MC.paint_bytes()))
    raw, stdout = run_harness_files(exe, tmp_path, header, *arrays)
    out = {"color": raw[:12 * n].view(F32).reshape(H, W, 3)}
    at = 12 * n
    if fb:
        out["fb"], at = raw[at:at + 4 * n].reshape(H, W, 4), at + 4 * n
    if aov:
        out["ids"], at = raw[at:at + n].reshape(H, W), at + n
    if summary:
        out["summary"], at = tuple(int(v) for v in raw[at:at + 16].view(np.uint32)), at + 16
    assert at == raw.size and int(stdout.split()[0]) >= 4 * n
    return out


def _assert_frame(got, want, what):
    assert np.array_equal(R.bits(got["color"]), R.bits(want[0])), what
    if "fb" in got:
        assert np.array_equal(got["fb"], R.bgra8(want[0])), what
    if "ids" in got:
        assert np.array_equal(got["ids"], want[1]), what
    if "summary" in got:
        assert got["summary"] == want[2], what


@pytest.mark.parametrize("i", range(len(MC.FIELD_BOXES)))
def test_the_field_code_on_the_host_equals_the_restatement(harness, tmp_path, i):
    origin, dims = MC.FIELD_BOXES[i]
    world = MC.terrain_world()
    want = _field(i)
    # several task cuts: one row per task, a cut that divides nothing, the three the launch picks from, the whole height in one task
    for seg in (1, 5, 16, 32, 64, 1000) if dims[0] * dims[1] * dims[2] < 100000 else (7, 16, 64):
        got = _run_field(harness, tmp_path, world, origin, dims, MC.RULES, MC.paint_bytes(), MC.PAINT_BOX, seg=seg)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], (i, seg)
    got = _run_field(harness, tmp_path, world, origin, dims, MC.RULES, seg=64, mis=1 + i % 3)  # byte stores whatever the width
    assert np.array_equal(got[0], _field(i, paint=False)[0]) and got[1] == _field(i, paint=False)[1], i


def test_the_field_code_on_the_host_at_every_brick_edge(harness, tmp_path):
    """the same world as 16- and 32-voxel bricks, padded with empty space to eight cells per axis"""
    origin, dims = (-4, 10, 2), (72, 50, 5)
    want = M.material_field_np(MC.terrain_world(), origin, dims, MC.RULES, MC.paint_bytes(), MC.PAINT_BOX)
    for factor in (16, 32):
        edge = 8 * factor
        world = np.zeros((edge, edge, edge), bool)
        world[:64, :64, :64] = MC.terrain_world()
        got = _run_field(harness, tmp_path, world, origin, dims, MC.RULES, MC.paint_bytes(), MC.PAINT_BOX, factor=factor)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], factor


@pytest.mark.parametrize("W,H,ortho,pose", MC.FRAME_CASES)
def test_the_frame_code_on_the_host_equals_the_restatement(harness, tmp_path, W, H, ortho, pose):
    case = MC.frame_case(W, H, ortho, pose)
    what = (W, H, ortho, pose)
    _assert_frame(_run_frame(harness, tmp_path, case), _frame(W, H, ortho, pose), what)
    _assert_frame(_run_frame(harness, tmp_path, case, alias=True, cus=1), _frame(W, H, ortho, pose), (what, "alias"))
    _assert_frame(_run_frame(harness, tmp_path, case, fb=False, aov=False, summary=False), _frame(W, H, ortho, pose), (what, "bare"))
    _assert_frame(_run_frame(harness, tmp_path, case, with_atlas=False, paint=False), _frame(W, H, ortho, pose, with_atlas=False, paint=False),
                  (what, "no atlas, no paint"))
    _assert_frame(_run_frame(harness, tmp_path, case, shift=0, n_tiles=1), _frame(W, H, ortho, pose, shift=0, n_tiles=1), (what, "T = 1"))
    _assert_frame(_run_frame(harness, tmp_path, case, shift=6, n_tiles=3, told_tiles=2),
                  _frame(W, H, ortho, pose, shift=6, n_tiles=3, told_tiles=2), (what, "T = 64, a tile withheld"))


def test_the_hand_derived_scenes_through_the_harness(harness, tmp_path):
    w = np.zeros(MC.WORLD, bool)
    w[4, 3:10, 4] = True
    paint = np.array([50, 0, 60], np.uint8).reshape(1, 3, 1)
    got = _run_field(harness, tmp_path, w, (4, 0, 4), (1, 12, 1), THREE, paint, ((4, 7, 4), (1, 3, 1)))
    assert got[0][0, :, 0].tolist() == [0, 0, 0, 3, 3, 3, 3, 50, 2, 60, 0, 0] and got[1][:3] == (7, 2, 1)
    w = np.zeros(MC.WORLD, bool)
    w[4, 20, 4] = True
    cam = tuple(np.asarray(v, F32) for v in ((-10.0, 20.25, 4.25), *MC.VIEWS["+x"]))
    o, d = R.primary_rays(16, 16, *cam, ortho=True, ortho_size=(4.0, 4.0))
    hit = MC.march_hits(w, o, d)
    case = dict(world=w, color=np.ones((16, 16, 3), F32), hit=hit, keys=R.keys_np(hit, MC.WORLD, o, d), o=o, d=d)
    got = _run_frame(harness, tmp_path, case, rules=THREE, paint=False, pal=MC.plain_palette(None, {1: (0, 0, 0)}), atl=QUAD)
    assert got["summary"] == (4, 0, 4, 4)
    seen = {tuple(got["color"][y, x].tolist()) for y, x in np.argwhere(got["ids"] == 1)}
    assert seen == {RED, GREEN, BLUE, YELLOW}
    (y, x), = [(y, x) for y, x in np.argwhere(got["ids"] == 1) if o[y, x, 1] < 20.5 and o[y, x, 2] < 4.5]
    assert tuple(got["color"][y, x].tolist()) == BLUE  # y low, z low: the bottom row's first texel


def test_the_harness_under_sanitizers(tmp_path):
    """the harness's own main, stand-alone, under ASan and UBSan"""
    exe = str(tmp_path / "material_check_san")
    root = helpers.ROOT
    tools, oracle = os.path.join(root, "tests", "tools"), os.path.join(root, "oracle")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(tools, "hoststub"), "-I" + oracle, "-o", exe, os.path.join(tools, "material_check.cpp"),
                        "-x", "c", *[os.path.join(oracle, f) for f in ("vxo_trace.c", "vxo_world.c", "vxo_render.c")], "-lm", "-lpthread", "-w"],
                       capture_output=True, text=True)
    if r.returncode != 0 and any(s in r.stderr.lower() for s in ("sanitize", "asan", "ubsan")):
        pytest.skip("no sanitizer runtime for the host compiler")
    assert r.returncode == 0, r.stderr[-2000:]
    for i in (1, 3, 7):
        origin, dims = MC.FIELD_BOXES[i]
        got = _run_field(exe, tmp_path, MC.terrain_world(), origin, dims, MC.RULES, MC.paint_bytes(), MC.PAINT_BOX, seg=9, mis=i % 2)
        assert np.array_equal(got[0], _field(i)[0]) and got[1] == _field(i)[1]
    for W, H, ortho, pose in ((65, 9, False, "up"), (64, 4, True, "zero"), (257, 3, True, "slant")):
        _assert_frame(_run_frame(exe, tmp_path, MC.frame_case(W, H, ortho, pose), shift=6, n_tiles=3), _frame(W, H, ortho, pose, shift=6, n_tiles=3), pose)


# ---- the limits and the order of the refusals ----------------------------------------------------------------------------
def test_limits_and_refusal_order(tmp_path_factory):
    exe = build_harness(tmp_path_factory, "material_args_check")
    out = run_harness(exe)
    source = open(os.path.join(helpers.ROOT, "tests", "tools", "material_args_check.cpp")).read()
    assert int(out.split()[0]) >= len(re.findall(r"\bCHECK\(", source)) - 1, out  # every CHECK of the program ran (loops: more than once)


def test_exports_and_abi_version():
    import voxelengine_amd as vx
    for name in ("vxrt_material_field", "vxrt_material_field_host", "vxrt_material_frame"):
        assert name in vx.EXPORTS
    header = open(os.path.join(helpers.ROOT, "include", "vxrt.h")).read()
    for name in ("vxrt_material_field", "vxrt_material_field_host", "vxrt_material_frame"):
        assert re.search(r"\bint %s\(" % name, header)
    assert re.search(r"#define VXRT_ABI_VERSION 3\b", header)
