"""CPU checks of voxel light fields (include/vxrt.h, vxrt_light_field): the restatements of tests/ref_light.py against each
other, against brute force and on the hand-derived cases of tests/light_cases.py, on worlds whose fields use the whole
scale, and the kernels' light code (csrc/vxrt_light.hpp) compiled for the host (tests/tools/light_check.cpp) against them
-- levels and summary bit-equal, every index checked -- with the workspace formula and the limits of the arguments."""
import ctypes as C

import numpy as np
import pytest

from tests import light_cases as LC
from tests import ref_light as R
from tests.helpers import build_harness, run_harness_files

WIDTHS = (1, 4, 5, 36, 37, 100)  # dims[0]: halo rows of 29, 32, 33, 64, 65 and 128 voxels


def _both(world, origin, dims, emitters=None, channels=R.SKY | R.BLOCK):
    """the dilation and the relaxation, asserted equal; returns the first"""
    a = R.light_field(world, origin, dims, emitters, channels)
    b = R.light_field_relax(world, origin, dims, emitters, channels)
    assert np.array_equal(a["levels"], b["levels"]) and a["summary"] == b["summary"], (origin, dims, channels)
    s = a["summary"]
    assert s[0] + sum(s[2]) == s[0] + sum(s[3]) == dims[0] * dims[1] * dims[2]
    return a


def _emitters(rng, lo, hi, n, sure=None):
    """n random entries in the box lo .. hi, levels 0 .. 16 (so some are invalid), some doubled, one certainly invalid and one
    certainly far, `sure` appended"""
    e = [(*(int(rng.integers(lo[k], hi[k])) for k in range(3)), int(rng.integers(0, 17))) for _ in range(n)]
    e += e[:max(n // 8, 1)] + [(lo[0], lo[1], lo[2], 16), (hi[0] + 100, hi[1], hi[2], 7)]
    return e + ([sure] if sure else [])


def _lamp_spot(world, origin, dims):
    """an empty voxel of the world inside the box, for an emitter that is certainly used"""
    lo = [max(o, 0) for o in origin]
    hi = [min(o + d, s) for o, d, s in zip(origin, dims, world.shape)]
    free = np.argwhere(~world[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
    return tuple(int(v) + l for v, l in zip(free[len(free) // 2], lo))


# ---- the restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [R.SKY, R.BLOCK, R.SKY | R.BLOCK])
def test_the_restatements_agree_on_random_grids(channels):
    rng = np.random.default_rng(channels)
    for density, origin, dims in [(0.45, (3, 20, 2), (20, 17, 19)), (0.2, (-6, -4, 30), (30, 9, 12)), (0.6, (10, 10, 10), (9, 9, 9)),
                                  (0.45, (60, 40, 60), (8, 12, 8)), (0.3, (100, 0, 0), (4, 5, 6))]:
        w = R.leaky_roof_world(rng, density=density)
        e = _emitters(rng, [o - 20 for o in origin], [o + d + 20 for o, d in zip(origin, dims)], 30)
        _both(w, origin, dims, e, channels)


def test_the_restatements_equal_brute_force_and_a_wider_halo_changes_nothing():
    """dense worlds keep the searches short; the last box lies half outside a small world, in open air"""
    rng = np.random.default_rng(9)
    for edge, density, origin, dims in [(40, 0.6, (17, 18, 17), (5, 5, 5)), (40, 0.5, (16, 20, 16), (3, 4, 3)),
                                        (40, 0.65, (14, 17, 15), (8, 8, 8)), (12, 0.3, (-1, 5, 4), (2, 3, 2))]:
        w = rng.random((edge, edge, edge)) < density
        w[:, edge * 2 // 3, :] = rng.random((edge, edge)) < 0.9
        x, y, z = _lamp_spot(w, origin, dims)
        e = [(x, y, z, 15), (x + 1, y, z, 9), (x, y + 2, z + 1, 1), (x - 3, y + 9, z, 12), (x + 60, y, z, 8), (x, y, z, 0)]
        a = _both(w, origin, dims, e)
        b = R.light_field_brute(w, origin, dims, e)
        assert np.array_equal(a["levels"], b["levels"]) and a["summary"] == b["summary"]
        c = R.light_field_brute(w, origin, dims, e, halo=20)  # far is the one count that depends on the halo
        assert np.array_equal(b["levels"], c["levels"]) and b["summary"][:6] == c["summary"][:6]
        assert a["summary"][1] < dims[0] * dims[1] * dims[2] or edge == 12


def _leaky():
    """the recipe of the contract's tests: noise of density 0.45 in 64 x 48 x 64 with a y-layer that is 90 % solid, a box
    that straddles the layer, starts at negative coordinates and ends beyond the world; 40 random emitters and one of level
    15 in a known empty voxel"""
    rng = np.random.default_rng(1)
    w = R.leaky_roof_world(rng)
    o, d = (-5, 10, -3), (74, 30, 70)
    e = _emitters(rng, (-10, 5, -10), (70, 45, 70), 40, sure=(*_lamp_spot(w, o, d), 15))
    return w, o, d, e


def test_leaky_roof_worlds_use_the_whole_scale():
    w, o, d, e = _leaky()
    assert not w[e[-1][:3]] and e[-1][3] == 15
    r = _both(w, o, d, e)
    hist_sky, hist_block = r["summary"][2], r["summary"][3]
    print("sky", hist_sky, "block", hist_block)
    assert all(n > 0 for n in hist_sky), hist_sky      # every level 0 .. 15 occurs in the sky channel
    assert all(n > 0 for n in hist_block), hist_block  # and in the block channel
    assert min(r["summary"][6:10]) > 0                 # and every class of emitter


def test_hand_derived_cases_on_the_restatements():
    for case in LC.all_cases():
        for channels in (R.SKY, R.BLOCK, R.SKY | R.BLOCK):
            LC.check(case, _both(case["world"], case["origin"], case["dims"], case["emitters"], channels), channels)
    for case in (LC.u_shaped_corridor(), LC.sky_hole_outside_the_box(14), LC.sky_hole_outside_the_box(15)):
        LC.check(case, R.light_field_brute(case["world"], case["origin"], case["dims"], case["emitters"]))


# ---- the kernels' light code on the host ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "light_check")


def _run_harness(harness, tmp_path, world, factor, origin, dims, emitters, channels):
    from oracle import vxo
    X, Y, Z = world.shape
    rows = np.zeros((0, 4), np.int32) if emitters is None else np.asarray(emitters, np.int32).reshape(-1, 4)
    header = [0, factor, X, Y, Z, *origin, *dims, channels, len(rows)]
    raw, _ = run_harness_files(harness, tmp_path, header, vxo.dense_from_voxels(world), rows)
    n = dims[0] * dims[1] * dims[2]
    assert raw.size == 4 * R.SUMMARY_WORDS + n
    levels = raw[4 * R.SUMMARY_WORDS:].reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)
    return {"levels": levels, "summary": R.summary_from_words(raw[:4 * R.SUMMARY_WORDS].copy())}


def _assert_harness(harness, tmp_path, world, factor, origin, dims, emitters=None, channels=R.SKY | R.BLOCK):
    want = R.light_field(world, origin, dims, emitters, channels)
    got = _run_harness(harness, tmp_path, world, factor, origin, dims, emitters, channels)
    assert np.array_equal(got["levels"], want["levels"]), (origin, dims, channels)
    assert got["summary"] == want["summary"], (origin, dims, channels)
    return got


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    for case in LC.all_cases():
        for channels in (R.SKY, R.BLOCK, R.SKY | R.BLOCK):
            got = _assert_harness(harness, tmp_path, case["world"], 8, case["origin"], case["dims"], case["emitters"], channels)
            LC.check(case, got, channels)


@pytest.mark.parametrize("factor,edge", [(8, 64), (16, 128), (32, 256)])
def test_host_code_equals_the_reference_on_leaky_roofs(harness, tmp_path, factor, edge):
    """brick edges 8, 16 and 32; dims[0] of 1, 4, 5, 36, 37 and 100; origins negative, unaligned and past the far faces;
    emitters of every class, with duplicates.  At brick edge 8 every box runs each channel alone and both; at 16 and 32 a box
    runs one mask, the six boxes taking the three masks in turn"""
    rng = np.random.default_rng(factor)
    w = R.leaky_roof_world(rng, shape=(edge, edge, edge), roof_y=edge // 2)
    roof = edge // 2
    boxes = [((3, roof - 9, 5), (1, 20, 9)), ((-7, roof - 4, -3), (4, 12, 11)), ((edge - 3, roof - 12, 9), (5, 17, 6)),
             ((11, roof - 10, edge - 20), (36, 15, 30)), ((-20, roof - 6, 17), (37, 13, 5)), ((edge - 70, roof - 8, 1), (100, 11, 7))]
    assert tuple(d[0] for _, d in boxes) == WIDTHS
    for i, (o, d) in enumerate(boxes):
        e = _emitters(rng, [v - 20 for v in o], [v + s + 20 for v, s in zip(o, d)], 24, sure=(*_lamp_spot(w, o, d), 15))
        for channels in ((R.SKY, R.BLOCK, R.SKY | R.BLOCK) if factor == 8 else (1 + i % 3,)):
            got = _assert_harness(harness, tmp_path, w, factor, o, d, e, channels)
            if channels & R.BLOCK:
                assert got["summary"][6] > 0 and got["summary"][9] > 0


def test_host_code_on_the_world_that_uses_the_whole_scale(harness, tmp_path):
    w, o, d, e = _leaky()
    world = np.zeros((64, 64, 64), bool)
    world[:, :48, :] = w  # brick edge 8 needs 64 voxels per axis: 16 empty rows on top change nothing
    got = _assert_harness(harness, tmp_path, world, 8, o, d, e)
    assert got["summary"] == R.light_field(w, o, d, e)["summary"]
    assert all(n > 0 for n in got["summary"][2]) and all(n > 0 for n in got["summary"][3])


def _layout(harness, tmp_path, origin, dims, channels):
    raw, _ = run_harness_files(harness, tmp_path, [1, 8, 64, 64, 64, *origin, *dims, channels, 0])
    with_o, without = (int(v) for v in np.frombuffer(raw[:8].tobytes(), np.uint32))
    return bool(with_o), bool(without), int(np.frombuffer(raw[8:16].tobytes(), np.uint64)[0])


def test_layout_accepts_the_last_origin_whose_halo_fits_int32(harness, tmp_path):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    for dims in [(8, 8, 8), (1, 3, 70), (1, 1, 1), (33, 2, 2)]:
        for k in range(3):
            for edge, ok in [(lo + 14, True), (lo + 13, False), (hi - dims[k] - 14, True), (hi - dims[k] - 13, False)]:
                origin = [0, 0, 0]
                origin[k] = edge
                assert _layout(harness, tmp_path, origin, dims, 3)[:2] == (ok, True), (dims, k, edge)
    for channels, ok in [(0, False), (1, True), (2, True), (3, True), (4, False), (-1, False)]:
        assert _layout(harness, tmp_path, (0, 0, 0), (8, 8, 8), channels)[:2] == (ok, ok)


def _expect_bytes(d, channels):  # the formula of include/vxrt.h
    r = lambda n: (n + 255) // 256 * 256
    h = [v + 28 for v in d]
    wh = (h[0] + 31) // 32
    P = 4 * wh * h[1] * h[2]
    n, s, b = bin(channels).count("1"), channels & 1, channels >> 1 & 1
    return r(P) * (1 + 6 * n) + s * r(4 * wh * h[2]) + b * 8 * 65536


def test_light_symbols_exported_and_workspace_bytes(harness, tmp_path):
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_light_workspace_bytes", "vxrt_light_field", "vxrt_light_field_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    ws = lambda d, c: int(lib.vxrt_light_workspace_bytes((C.c_int32 * 3)(*d), c))
    for bad in [(0, 8, 8), (8, -1, 8), (1 << 10, 1 << 10, (1 << 8) + 1), (1 << 29, 1, 1)]:
        assert ws(bad, 3) == 0
    for bad in (0, 4, 7, 1 << 31):
        assert ws((8, 8, 8), bad) == 0
    assert ws((1 << 14, 1 << 14, 1), 3) > 0 and ws((1, 1 << 14, 1 << 14), 3) > 0
    assert ws((1, 1, 1 << 28), 3) == 0 and ws((1, 1, 1 << 26), 3) > 0  # the halo box, 29 x 29 x (dims[2] + 28), against 2^36 voxels
    assert lib.vxrt_light_workspace_bytes(None, 3) == 0
    for d in [(1, 1, 1), (4, 7, 5), (5, 3, 9), (36, 2, 2), (37, 64, 8), (100, 9, 3), (256, 128, 256), (1024, 256, 1024)]:
        for channels in (1, 2, 3):
            want = _expect_bytes(d, channels)
            assert ws(d, channels) == want, (d, channels)
            if d[0] <= 100:
                assert _layout(harness, tmp_path, (0, 0, 0), d, channels)[2] == want
    assert ws((256, 128, 256), 3) <= 3 * 256 * 128 * 256  # 13 bit planes of a halo 1.5 times the box: under 3 bytes per voxel
    o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    assert lib.vxrt_light_field(None, o3, d3, None, 0, 3, None, None, None, None) == -1
    assert lib.vxrt_light_field_host(None, o3, d3, None, 0, 3, None, None) == -1
    assert (vx.LIGHT_SKY, vx.LIGHT_BLOCK, vx.LIGHT_MAX, vx.LIGHT_MAX_EMITTERS) == (1, 2, 15, 65536)
    assert (R.SKY, R.BLOCK, R.MAX, R.HALO, R.MAX_EMITTERS) == (vx.LIGHT_SKY, vx.LIGHT_BLOCK, vx.LIGHT_MAX, vx.LIGHT_MAX - 1, 65536)
