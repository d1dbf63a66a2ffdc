"""CPU checks of the light on frames (include/vxrt.h, vxrt_light_frame): the two restatements of tests/ref_light_frame.py
against each other on the random cases of tests/light_frame_cases.py, what those cases exercise (checked on the restatement
alone, so that a case set cannot hide a branch), hand-derived cases with the expected numbers written out, the kernel's
per-pixel code (csrc/vxrt_light_frame.hpp) compiled for the host (tests/tools/lightframe_check.cpp) against the restatement
-- colours, BGRA8, terms and summary bit-equal, every index checked -- and the limits and the order of the refusals
(tests/tools/lightframe_args_check.cpp)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import light_frame_cases as LC
from tests import ref_denoise as R
from tests import ref_light_frame as LF
from tests.helpers import build_harness, run_harness, run_harness_files

F32 = np.float32
BOTH = LF.SMOOTH | LF.OCCLUSION
DYADIC = dict(sky_floor=0.25, block_color=(1.0, 0.5, 0.25), ao_curve=(0.25, 0.5, 0.75, 0.875), outside_level=0xF0)


@functools.lru_cache(maxsize=None)
def _case(W, H, ortho, pose):
    return LC.random_case(W, H, ortho, pose)


@functools.lru_cache(maxsize=None)
def _want(W, H, ortho, pose, flags=BOTH, levels=True):
    out = LC.run_case(_case(W, H, ortho, pose), flags, levels=levels)
    for a in out[:2]:
        a.setflags(write=False)
    return out


# ---- the restatements against each other -------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,ortho,pose", LC.CASES)
def test_the_restatements_agree(W, H, ortho, pose):
    case = _case(W, H, ortho, pose)
    big = W * H > 4000
    for flags, levels in ((BOTH, True),) if big else [(f, True) for f in LC.FLAG_SETS] + [(BOTH, False)]:
        a = _want(W, H, ortho, pose, flags, levels)
        b = LC.run_case(case, flags, scalar=True, levels=levels)
        what = (W, H, ortho, pose, flags, levels)
        assert np.array_equal(R.bits(a[0]), R.bits(b[0])), what
        assert np.array_equal(R.bits(a[1]), R.bits(b[1])), what
        assert a[2] == b[2], what
        hit, in_box, occluded, dark = a[2]
        assert hit == int(a[3]["hit"].sum()) and in_box <= hit and occluded <= hit and dark <= hit and (levels or in_box == 0)
        miss = ~a[3]["hit"]
        assert np.array_equal(R.bits(a[0][miss]), R.bits(case["color"][miss])) and not a[1][miss].any()
    print("light frame random case", W, H, ortho, pose, "hit, in_box, occluded, dark", _want(W, H, ortho, pose)[2])


def test_the_random_cases_reach_every_branch():
    """on the restatement alone, over the case set: every `open` value and every `cnt`, both clamps of the position on the
    face and positions inside it, the centre fallback, front cells in the box, outside it, and faces with some of their nine
    cells inside the box and some outside, a front cell outside the world, miss pixels -- and every flag changes something"""
    seen_open, seen_cnt = set(), set()
    flags_seen = dict(low=0, high=0, interior=0, centre=0, front_in=0, front_out=0, partial=0, outside_world=0, miss=0)
    for W, H, ortho, pose in LC.CASES:
        case = _case(W, H, ortho, pose)
        out, terms, summary, info = _want(W, H, ortho, pose)
        hit = info["hit"]
        seen_open |= set(np.unique(info["open"][hit]).tolist())
        seen_cnt |= set(np.unique(info["cnt"][hit]).tolist())
        proper = hit & ~info["centre"]
        flags_seen["low"] += int((proper & info["low"]).sum())
        flags_seen["high"] += int((proper & info["high"]).sum())
        flags_seen["interior"] += int((proper & info["interior"]).sum())
        flags_seen["centre"] += int((hit & info["centre"]).sum())
        flags_seen["front_in"] += int((hit & info["front_in_box"]).sum())
        flags_seen["front_out"] += int((hit & ~info["front_in_box"]).sum())
        flags_seen["partial"] += int((hit & (info["cells_in_box"] > 0) & (info["cells_in_box"] < 9)).sum())
        flags_seen["outside_world"] += int((hit & info["front_outside_world"]).sum())
        flags_seen["miss"] += int((~hit).sum())
        assert int(((case["keys"] == 0) & (case["hit"] >= 0)).sum()) > 0 or W * H < 100  # indices beyond the world
        if pose == "zero":
            assert (info["centre"] | ~hit).all() and hit.sum() > 10
        if W * H > 2000:
            for flags in LC.FLAG_SETS[1:]:
                other = _want(W, H, ortho, pose, flags)
                assert not np.array_equal(R.bits(other[0]), R.bits(out)) and other[2][:3] == summary[:3]
            bare = _want(W, H, ortho, pose, BOTH, False)
            assert not np.array_equal(R.bits(bare[0]), R.bits(out)) and bare[2][1] == 0 and summary[1] > 0
    print("light frame branches", sorted(seen_open), sorted(seen_cnt), flags_seen)
    assert seen_open == {0, 1, 2, 3} and seen_cnt == {1, 2, 3, 4}
    assert all(v > 0 for v in flags_seen.values()), flags_seen


# ---- hand-derived cases ------------------------------------------------------------------------------------------------
def test_a_flat_plate_under_full_sky():
    """no levels, outside_level 0xF0: every cell has sky 15 and block 0, every corner has four members and three open
    neighbours: S = 60 / 4 / 15 = 1, Bk = 0, A = ao_curve[3] = 0.875, ks = 0.25 + 0.75 * 1 = 1, out = 0.5 * 1 * 0.875"""
    out, terms, summary, info = LC.lit_from_above(LC.plate_world(), params=DYADIC)
    assert summary == (64, 0, 0, 0)
    assert (terms[..., 0] == 1.0).all() and (terms[..., 1] == 0.0).all() and (terms[..., 2] == 0.875).all()
    assert (out == 0.4375).all()
    assert (info["cnt"] == 4).all() and (info["open"] == 3).all() and not info["centre"].any()
    # a camera half a voxel to the side: u = 1 exactly -- the same numbers, all corners being equal
    out2, terms2, _, info2 = LC.lit_from_above(LC.plate_world(), params=DYADIC, cam=LC.top_camera(0.5, 0.0))
    assert np.array_equal(out2, out) and np.array_equal(terms2, terms)


def test_a_pillar_on_the_plate():
    """one voxel (3, 11, 3) on the plate, full sky.  Pixel (2, 3) has it at i = +1: the corners (1, 0) and (1, 1) have s1, two
    open neighbours (0.75) and three members; the others 0.875; at u = w = 0.5: A = 0.875 + 0.5 * (0.75 - 0.875) = 0.8125 on
    both rows.  Pixel (2, 2) has it at the diagonal: corner (1, 1) alone has s3: rows 0.875 and 0.8125, A = 0.84375.  The pillar's
    own top is open.  With a darker cell (1, 11, 3) of sky 3 the corners (0, 0) and (0, 1) of pixel (2, 3) average
    (15 + 3 + 15 + 15) / 4 = 12 and the other two (15 + 15 + 15) / 3 = 15: LS = 13.5"""
    world = LC.plate_world([(3, 11, 3)])
    out, terms, summary, info = LC.lit_from_above(world, params=DYADIC)
    assert summary == (64, 0, 8, 0)
    assert terms[3, 2, 2] == 0.8125 and terms[3, 4, 2] == 0.8125 and terms[2, 3, 2] == 0.8125 and terms[4, 3, 2] == 0.8125
    assert terms[2, 2, 2] == 0.84375 and terms[4, 4, 2] == 0.84375 and terms[3, 3, 2] == 0.875 and terms[0, 0, 2] == 0.875
    assert out[3, 2, 0] == 0.5 * 0.8125 and out[2, 2, 0] == 0.5 * 0.84375 and (terms[..., 0] == 1.0).all()
    assert info["cnt"][3, 2].tolist() == [4, 3, 4, 3] and info["open"][3, 2].tolist() == [3, 2, 3, 2]  # corners (0,0) (1,0) (0,1) (1,1)
    assert info["cnt"][2, 2].tolist() == [4, 4, 4, 3] and info["open"][2, 2].tolist() == [3, 3, 3, 2]
    box = ((0, 11, 0), (8, 1, 8))
    levels = np.full(box[1], 0xF0, np.uint8)
    levels[1, 0, 3] = 0x30
    out, terms, summary, _ = LC.lit_from_above(world, levels, box, DYADIC)
    assert summary == (64, 63, 8, 0)  # the pillar's own front cell lies above the box
    S = F32(13.5) / F32(15)
    assert terms[3, 2, 0] == S and terms[3, 2, 1] == 0.0 and terms[3, 2, 2] == 0.8125
    assert out[3, 2, 0] == (F32(0.5) * (F32(0.25) + F32(0.75) * S)) * F32(0.8125)
    # SMOOTH off: the front cell's own level, 15; OCCLUSION off: A = 1; both off: the colour as it was under full sky
    flat = LC.lit_from_above(world, levels, box, dict(DYADIC, flags=LF.OCCLUSION))
    assert flat[1][3, 2, 0] == 1.0 and flat[1][3, 2, 2] == 0.8125 and flat[1][3, 1, 0] == F32(3) / F32(15) and flat[2] == summary
    plain = LC.lit_from_above(world, levels, box, dict(DYADIC, flags=LF.SMOOTH))
    assert plain[1][3, 2, 0] == S and (plain[1][..., 2] == 1.0).all() and plain[2] == summary
    neither = LC.lit_from_above(world, levels, box, dict(DYADIC, flags=0))
    assert neither[0][3, 2, 0] == 0.5 and (neither[1][..., 2] == 1.0).all() and neither[2] == summary


def test_light_does_not_leak_through_a_closed_corner():
    """pixel (2, 2) stands in an inner corner: (3, 11, 2) and (2, 11, 3) are solid, the cell (3, 11, 3) behind them is empty and
    the only lit cell (0xFF).  Corner (1, 1) has s1 && s2: its one member is the front cell (cnt = 1, open = 0), nothing of
    the bright cell arrives: S = Bk = 0, the pixel is dark.  A: rows 0.875 .. 0.75 and 0.75 .. 0.25: 0.8125 and 0.5, 0.65625;
    out = 0.5 * 0.25 * 0.65625"""
    world = LC.plate_world([(3, 11, 2), (2, 11, 3)])
    box = ((0, 11, 0), (8, 1, 8))
    levels = np.zeros(box[1], np.uint8)
    levels[3, 0, 3] = 0xFF
    out, terms, summary, info = LC.lit_from_above(world, levels, box, dict(DYADIC, outside_level=0))
    assert info["cnt"][2, 2].tolist() == [4, 3, 3, 1] and info["open"][2, 2].tolist() == [3, 2, 2, 0]
    assert terms[2, 2].tolist() == [0.0, 0.0, 0.65625] and (out[2, 2] == 0.08203125).all()
    # the bright cell's own pixel (3, 3): corner (0, 0) is the closed one seen from inside: its only member is the bright cell
    assert info["cnt"][3, 3].tolist() == [1, 3, 3, 4] and terms[3, 3, 0] > 0 and terms[3, 3, 1] > 0
    lit = terms[..., 0] > 0
    # (y, x): the bright cell, its three open sides, and the two cells that see it past one pillar (s1 or s2 alone closes nothing)
    assert [(int(y), int(x)) for y, x in zip(*np.nonzero(lit))] == [(2, 4), (3, 3), (3, 4), (4, 2), (4, 3), (4, 4)]
    assert summary[0] == 64 and summary[3] == 64 - 6
    # if the corner leaked, corner (1, 1) of pixel (2, 2) would hold 15 / 2: restate that to show the case can tell
    assert levels[3, 0, 3] >> 4 == 15 and not world[3, 11, 3]


def test_no_levels_and_a_face_on_the_world_boundary():
    """a wall at x = 0 seen from outside the world along +x: the front cells lie at x = -1, outside the world (empty) but
    inside a box that starts at x = -2: their level is the box's byte (sky 8), S = 8 / 15.  Without levels the same cells
    take outside_level: S = 1, in_box = 0"""
    world = np.zeros(LC.WORLD, bool)
    world[0, :, :] = True
    X, Y, Z = LC.WORLD
    cam = ((-10.0, 8.5, 4.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))  # right = +z, up = +y: pixel (x, y) sees voxel (0, y + 4, x)
    hit = np.array([[0 + X * ((py + 4) + Y * px) for px in range(LC.HW)] for py in range(LC.HH)], np.int64)
    color = np.full((LC.HH, LC.HW, 3), 0.5, F32)
    box = ((-2, 0, -1), (2, 64, 66))  # (from z = -1 on: the nine cells of the pixels of column 0 reach there)
    levels = np.full(box[1], 0x80, np.uint8)
    kw = dict(ortho=True, ortho_size=LC.WINDOW)
    for scalar in (False, True):
        out, terms, summary = LF.light_frame(color, hit, cam, world, levels, box, DYADIC, scalar=scalar, **kw)[:3]
        assert summary == (64, 64, 0, 0)
        assert (terms[..., 0] == F32(8) / F32(15)).all() and (terms[..., 2] == 0.875).all()
        out, terms, summary = LF.light_frame(color, hit, cam, world, None, box, DYADIC, scalar=scalar, **kw)[:3]
        assert summary == (64, 0, 0, 0) and (terms[..., 0] == 1.0).all() and (out == 0.4375).all()
    info = LF.light_frame(color, hit, cam, world, levels, box, DYADIC, **kw)[3]
    assert info["front_outside_world"].all() and (info["open"] == 3).all()
    keys = R.keys_np(hit, LC.WORLD, *R.primary_rays(LC.HW, LC.HH, *cam, **kw))
    assert (keys == (0x80000000 | (0 << 26) | (1 << 25) | 0)).all()  # axis 0, toward, plane 0


def test_block_light_adds_its_colour():
    """one cell of block level 15 and sky 0 under a flat plate's pixel, sky_floor 0.25: the pixel over it averages its corners
    (15 + 0 + 0 + 0) / 4 = 3.75 each: Bk = 0.25, S = 0: out = (0.5 * 0.25 + block_color * 0.25) * 0.875"""
    box = ((0, 11, 0), (8, 1, 8))
    levels = np.zeros(box[1], np.uint8)
    levels[4, 0, 4] = 0x0F
    out, terms, summary, _ = LC.lit_from_above(LC.plate_world(), levels, box, dict(DYADIC, outside_level=0))
    assert terms[4, 4].tolist() == [0.0, 0.25, 0.875]
    assert out[4, 4].tolist() == [(0.125 + 1.0 * 0.25) * 0.875, (0.125 + 0.5 * 0.25) * 0.875, (0.125 + 0.25 * 0.25) * 0.875]
    assert summary == (64, 64, 0, 64 - 9)


# ---- the kernel's code on the host -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "lightframe_check")


def _run(exe, tmp_path, case, flags=BOTH, levels=True, fb=True, terms=True, summary=True, alias=False, cus=256, factor=8):
    from oracle import vxo
    H, W = case["keys"].shape
    n = W * H
    o, d = R.primary_rays(W, H, *case["cam"], ortho=case["ortho"], ortho_size=case["ortho_size"])
    p = case["params"]
    io = int(levels) | 2 * fb | 4 * terms | 8 * summary | 16 * alias
    header = [0, W, H, io, factor, *case["world"].shape, *case["box"][0], *case["box"][1], flags, p["outside_level"], cus, 0, 0, 0]
    arrays = [np.array([p["sky_floor"], *p["block_color"], *p["ao_curve"]], F32), vxo.dense_from_voxels(case["world"]), case["color"],
              case["keys"], case["hit"], o, d]
    if levels:
        arrays.append(np.ascontiguousarray(case["levels"].transpose(2, 1, 0)))  # region order: x fastest
    raw, stdout = run_harness_files(exe, tmp_path, header, *arrays)
    out = {"color": raw[:12 * n].view(F32).reshape(H, W, 3)}
    at = 12 * n
    if fb:
        out["fb"], at = raw[at:at + 4 * n].reshape(H, W, 4), at + 4 * n
    if terms:
        out["terms"], at = raw[at:at + 12 * n].view(F32).reshape(H, W, 3), at + 12 * n
    if summary:
        out["summary"], at = tuple(int(v) for v in raw[at:at + 16].view(np.uint32)), at + 16
    assert at == raw.size and int(stdout.split()[0]) >= 4 * n
    return out


def _assert_equal(got, want, what):
    color, terms, summary = want[:3]
    assert np.array_equal(R.bits(got["color"]), R.bits(color)), what
    if "fb" in got:
        assert np.array_equal(got["fb"], R.bgra8(color)), what
    if "terms" in got:
        assert np.array_equal(R.bits(got["terms"]), R.bits(terms)), what
    if "summary" in got:
        assert got["summary"] == summary, what


@pytest.mark.parametrize("W,H,ortho,pose", LC.CASES)
def test_the_kernel_code_on_the_host_equals_the_restatement(harness, tmp_path, W, H, ortho, pose):
    case = _case(W, H, ortho, pose)
    what = (W, H, ortho, pose)
    for flags in LC.FLAG_SETS:
        _assert_equal(_run(harness, tmp_path, case, flags), _want(W, H, ortho, pose, flags), (what, flags))
    _assert_equal(_run(harness, tmp_path, case, alias=True, cus=1), _want(W, H, ortho, pose), (what, "alias"))  # waves on many tiles
    _assert_equal(_run(harness, tmp_path, case, fb=False, terms=False, summary=False), _want(W, H, ortho, pose), (what, "bare"))
    _assert_equal(_run(harness, tmp_path, case, levels=False), _want(W, H, ortho, pose, BOTH, False), (what, "no levels"))


def test_the_kernel_code_on_the_host_at_every_brick_edge(harness, tmp_path):
    """the same world as 8-, 16- and 32-voxel bricks (the world's 64 voxels are two cells of 32: the tables want multiples
    of 8 cells, so the world is padded with empty space to 256 voxels per axis -- the hit indices are re-made for it)"""
    case = dict(_case(67, 35, False, "slant"))
    want = _want(67, 35, False, "slant")
    for factor in (16, 32):
        edge = 8 * factor
        world = np.zeros((edge, edge, edge), bool)
        world[:64, :64, :64] = case["world"]
        X, Y, Z = LC.WORLD
        h = case["hit"]
        inside = (h >= 0) & (h < X * Y * Z)
        v = (h % X, h // X % Y, h // (X * Y))
        moved = np.where(inside, v[0] + edge * (v[1] + edge * v[2]), np.where(h < 0, h, edge ** 3 + 7))
        padded = dict(case, world=world, hit=moved)
        # the front cells at x, y, z = 64 are now inside the world (and empty): nothing the restatement can tell apart
        _assert_equal(_run(harness, tmp_path, padded, factor=factor), LC.run_case(padded), factor)
        assert np.array_equal(R.bits(LC.run_case(padded)[0]), R.bits(want[0]))


def test_the_hand_derived_scenes_through_the_harness(harness, tmp_path):
    world = LC.plate_world([(3, 11, 2), (2, 11, 3)])
    box = ((0, 11, 0), (8, 1, 8))
    levels = np.zeros(box[1], np.uint8)
    levels[3, 0, 3] = 0xFF
    hit = LC.top_hits(world)
    cam = tuple(np.asarray(v, F32) for v in LC.top_camera())
    o, d = R.primary_rays(LC.HW, LC.HH, *cam, ortho=True, ortho_size=LC.WINDOW)
    case = dict(world=world, levels=levels, box=box, color=np.full((LC.HH, LC.HW, 3), 0.5, F32), hit=hit, keys=R.keys_np(hit, LC.WORLD, o, d),
                cam=cam, ortho=True, ortho_size=LC.WINDOW, params=dict(DYADIC, outside_level=0))
    got = _run(harness, tmp_path, case)
    _assert_equal(got, LC.run_case(case), "inner corner")
    assert got["terms"][2, 2].tolist() == [0.0, 0.0, 0.65625] and (got["color"][2, 2] == 0.08203125).all()


def test_the_harness_under_sanitizers(tmp_path):
    """the harness's own main, stand-alone, under ASan and UBSan"""
    exe = str(tmp_path / "lightframe_check_san")
    root = helpers.ROOT
    tools, oracle = os.path.join(root, "tests", "tools"), os.path.join(root, "oracle")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(tools, "hoststub"), "-I" + oracle, "-o", exe, os.path.join(tools, "lightframe_check.cpp"),
                        "-x", "c", *[os.path.join(oracle, f) for f in ("vxo_trace.c", "vxo_world.c", "vxo_render.c")], "-lm", "-lpthread", "-w"],
                       capture_output=True, text=True)
    if r.returncode != 0 and any(s in r.stderr.lower() for s in ("sanitize", "asan", "ubsan")):
        pytest.skip("no sanitizer runtime for the host compiler")
    assert r.returncode == 0, r.stderr[-2000:]
    for ortho in (False, True):
        _assert_equal(_run(exe, tmp_path, _case(67, 35, ortho, "slant")), _want(67, 35, ortho, "slant"), ortho)
    _assert_equal(_run(exe, tmp_path, _case(64, 1, True, "zero"), levels=False, alias=True), _want(64, 1, True, "zero", BOTH, False), "zero")


# ---- the limits and the order of the refusals ----------------------------------------------------------------------------
def test_limits_and_refusal_order(tmp_path_factory):
    exe = build_harness(tmp_path_factory, "lightframe_args_check")
    out = run_harness(exe)
    assert int(out.split()[0]) == 141, out  # every CHECK of the program ran
