"""CPU checks of exact distance fields (include/vxrt.h, vxrt_distance_field): the restatements of tests/ref_dist.py against
each other, against brute force and on hand-derived cases, and the kernels' distance code (csrc/vxrt_dist.hpp) compiled for
the host (tests/tools/dist_check.cpp) against them -- field and summary bit-equal, every index checked, the empty-space skip
on and off, the workspace formula and the limits of the origin."""
import ctypes as C

import numpy as np
import pytest

from tests import ref_dist as R
from tests.helpers import build_harness, run_harness_files

FAR = R.FAR


def _both(world, origin, dims, radius, mode):
    """both restatements, asserted equal; returns the numpy one"""
    a = R.distance_field(world, origin, dims, radius, mode)
    if R.have_scipy():
        b = R.distance_field_scipy(world, origin, dims, radius, mode)
        assert np.array_equal(a["dist2"], b["dist2"]) and a["summary"] == b["summary"]
    s = a["summary"]
    assert s[0] + s[1] + s[2] == dims[0] * dims[1] * dims[2] and s[3] <= radius * radius
    return a


# ---- the restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.TO_SOLID, R.TO_EMPTY])
def test_the_restatements_agree_on_random_grids(mode):
    rng = np.random.default_rng(3 + mode)
    for density, origin, dims, radius in [(0.01, (0, 0, 0), (24, 16, 24), 7), (0.3, (3, -2, 1), (21, 17, 19), 2),
                                          (0.0005, (-4, 0, -3), (30, 12, 9), 40), (0.5, (20, 20, 20), (9, 9, 9), 1),
                                          (0.002, (5, 30, 5), (4, 3, 2), 255), (0.1, (40, 40, 40), (5, 5, 5), 9)]:
        w = rng.random((24, 20, 24)) < (density if mode == R.TO_SOLID else 1 - density)
        _both(w, origin, dims, radius, mode)


@pytest.mark.parametrize("mode", [R.TO_SOLID, R.TO_EMPTY])
def test_the_restatements_equal_brute_force(mode):
    rng = np.random.default_rng(5 + mode)
    for density, origin, dims, radius in [(0.02, (0, 0, 0), (8, 7, 6), 5), (0.4, (-2, 3, 9), (7, 5, 6), 3), (0.01, (2, 2, 2), (3, 3, 3), 12)]:
        w = rng.random((12, 10, 12)) < density
        a, b = _both(w, origin, dims, radius, mode), R.distance_field_brute(w, origin, dims, radius, mode)
        assert np.array_equal(a["dist2"], b["dist2"]) and a["summary"] == b["summary"]


def _shells(dims, c, radius):
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1)
    d2 = ((g - np.asarray(c)) ** 2).sum(-1)
    return np.where(d2 <= radius * radius, d2, FAR).astype(np.uint16)


def _one_voxel():
    w = np.zeros((64, 64, 64), bool)
    w[30, 31, 32] = True
    return w, (18, 19, 20), (24, 24, 24), 9  # the box holds the whole ball around voxel (12, 12, 12) of it


def _check_one_voxel(r):
    assert np.array_equal(r["dist2"], _shells((24, 24, 24), (12, 12, 12), 9))
    n = R.ball_points(9)
    assert r["summary"][:4] == (1, n - 1, 24 ** 3 - n, 81) and n == 3071


def _floor(h=5):
    w = np.zeros((64, 64, 64), bool)
    w[:, :h, :] = True
    return w, (10, 0, 10), (20, 30, 20), 12, h


def _check_floor(r, h=5):
    y = np.arange(30)
    want = np.where(y < h, 0, np.where(y - h + 1 <= 12, (y - h + 1) ** 2, FAR)).astype(np.uint16)
    assert np.array_equal(r["dist2"], np.broadcast_to(want[None, :, None], (20, 30, 20)))


def _block(a=11, b=7, c=14):
    w = np.zeros((64, 64, 64), bool)
    w[20:20 + a, 30:30 + b, 10:10 + c] = True
    return w, (20, 30, 10), (a, b, c), 8


def _check_block(r, a=11, b=7, c=14):
    steps = lambda n: np.minimum(np.arange(n) + 1, n - np.arange(n))  # to the first empty voxel past the nearer face
    want = np.minimum(np.minimum(steps(a)[:, None, None], steps(b)[None, :, None]), steps(c)[None, None, :]) ** 2
    assert np.array_equal(r["dist2"], want.astype(np.uint16)) and r["summary"][0] == 0 and r["summary"][3] == 16


def _edge():
    return np.ones((64, 64, 64), bool), (-3, 50, 60), (20, 20, 10), 15


def _check_edge(r):
    x, y, z = np.arange(-3, 17), np.arange(50, 70), np.arange(60, 70)
    inside = lambda v: (v >= 0) & (v < 64)
    steps = lambda v: np.where(inside(v), np.minimum(v + 1, 64 - v), 0)  # the outside counts as empty
    want = np.minimum(np.minimum(steps(x)[:, None, None], steps(y)[None, :, None]), steps(z)[None, None, :]) ** 2
    assert np.array_equal(r["dist2"], want.astype(np.uint16))
    assert r["dist2"][3, 0, 0] == 1 and r["dist2"][10, 5, 0] == 16 and r["dist2"][0, 0, 0] == 0


def _check_all_far(r, n):
    assert (r["dist2"] == FAR).all() and r["summary"] == (0, 0, n, 0, 0)


def test_hand_derived_cases_on_the_restatements():
    w, o, d, rad = _one_voxel()
    _check_one_voxel(_both(w, o, d, rad, R.TO_SOLID))
    w, o, d, rad, h = _floor()
    _check_floor(_both(w, o, d, rad, R.TO_SOLID))
    w, o, d, rad = _block()
    _check_block(_both(w, o, d, rad, R.TO_EMPTY))
    w, o, d, rad = _edge()
    _check_edge(_both(w, o, d, rad, R.TO_EMPTY))
    w = np.zeros((64, 64, 64), bool)
    w[0, 0, 0] = True
    _check_all_far(_both(w, (30, 30, 30), (10, 9, 8), 12, R.TO_SOLID), 720)   # the nearest solid voxel is 18 away on every axis
    _check_all_far(_both(np.ones((64, 64, 64), bool), (20, 20, 20), (10, 9, 8), 12, R.TO_EMPTY), 720)
    # wholly outside the world: nothing solid in reach, everything empty
    _check_all_far(_both(np.ones((64, 64, 64), bool), (200, 0, 0), (5, 5, 5), 40, R.TO_SOLID), 125)
    assert _both(np.ones((64, 64, 64), bool), (200, 0, 0), (5, 5, 5), 40, R.TO_EMPTY)["summary"] == (125, 0, 0, 0, 0)


# ---- the kernels' distance code on the host -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "dist_check")


def _run_harness(harness, tmp_path, world, factor, origin, dims, radius, mode, skip=1):
    from oracle import vxo
    X, Y, Z = world.shape
    header = [0, factor, X, Y, Z, *origin, *dims, radius, mode, skip]
    raw, _ = run_harness_files(harness, tmp_path, header, vxo.dense_from_voxels(world))
    n = dims[0] * dims[1] * dims[2]
    s = np.frombuffer(raw[:16].tobytes(), np.uint32)
    total = int(np.frombuffer(raw[16:24].tobytes(), np.uint64)[0])
    live, tiles = (int(v) for v in np.frombuffer(raw[24:32].tobytes(), np.uint32))
    d2 = np.frombuffer(raw[32:32 + 2 * n].tobytes(), np.uint16).reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)
    assert tiles == -(-dims[0] // 64) * -(-dims[1] // 64) * -(-dims[2] // 64) and live <= tiles
    return {"dist2": d2, "summary": (int(s[0]), int(s[1]), int(s[2]), int(s[3]), total), "live": live, "tiles": tiles}


def _assert_harness(harness, tmp_path, world, factor, origin, dims, radius, mode, want=None):
    want = want or R.fast(world, origin, dims, radius, mode)
    got = _run_harness(harness, tmp_path, world, factor, origin, dims, radius, mode)
    assert np.array_equal(got["dist2"], want["dist2"]), (origin, dims, radius, mode)
    assert got["summary"] == want["summary"], (origin, dims, radius, mode)
    return got


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    w, o, d, rad = _one_voxel()
    _check_one_voxel(_assert_harness(harness, tmp_path, w, 8, o, d, rad, R.TO_SOLID))
    w, o, d, rad, h = _floor()
    _check_floor(_assert_harness(harness, tmp_path, w, 8, o, d, rad, R.TO_SOLID))
    w, o, d, rad = _block()
    _check_block(_assert_harness(harness, tmp_path, w, 8, o, d, rad, R.TO_EMPTY))
    w, o, d, rad = _edge()
    _check_edge(_assert_harness(harness, tmp_path, w, 8, o, d, rad, R.TO_EMPTY))
    w = np.zeros((64, 64, 64), bool)
    w[0, 0, 0] = True
    got = _assert_harness(harness, tmp_path, w, 8, (30, 30, 30), (10, 9, 8), 12, R.TO_SOLID)
    _check_all_far(got, 720)
    assert got["live"] == 0
    _check_all_far(_assert_harness(harness, tmp_path, np.ones((64, 64, 64), bool), 8, (200, 0, 0), (5, 5, 5), 40, R.TO_SOLID), 125)
    assert _assert_harness(harness, tmp_path, np.ones((64, 64, 64), bool), 8, (200, 0, 0), (5, 5, 5), 40, R.TO_EMPTY)["summary"] == \
        (125, 0, 0, 0, 0)


@pytest.mark.parametrize("mode", [R.TO_SOLID, R.TO_EMPTY])
@pytest.mark.parametrize("radius", [1, 2, 9, 40, 255])
def test_host_code_equals_the_reference_on_random_grids(harness, tmp_path, radius, mode):
    """densities 0.0005 .. 0.5 (of targets), dims[0] in {1, 31, 32, 33, 65}, origins negative and past the world, a box
    wholly outside it"""
    rng = np.random.default_rng(radius + 7 * mode)
    densities = [0.0005, 0.004, 0.05, 0.5, 0.02]
    small = radius > 40  # the halo of R = 255 is 510 voxels wider than the box on every axis
    boxes = [((0, 0, 0), (32, 20, 70)), ((-9, -7, 40), (65, 33, 30)), ((40, 50, 60), (31, 30, 9)), ((5, 70, 5), (1, 66, 7)),
             ((-300, 10, 10), (33, 5, 4))]
    for i, (density, (origin, dims)) in enumerate(zip(densities, boxes)):
        if small:  # the reference alone takes ten seconds and more on such a halo: two boxes, dims[0] = 65 and 1
            if i not in (1, 3):
                continue
            dims = tuple(min(v, 12) if k else v for k, v in enumerate(dims))
        w = rng.random((64, 64, 64)) < (density if mode == R.TO_SOLID else 1 - density)
        _assert_harness(harness, tmp_path, w, 8, origin, dims, radius, mode)


@pytest.mark.parametrize("factor,edge", [(16, 128), (32, 256)])
def test_host_code_on_larger_bricks(harness, tmp_path, factor, edge):
    rng = np.random.default_rng(factor)
    w = rng.random((edge, edge, edge)) < 0.001
    for mode in (R.TO_SOLID, R.TO_EMPTY):
        _assert_harness(harness, tmp_path, w if mode == R.TO_SOLID else ~w, factor, (edge - 50, -10, 3), (70, 40, 33), 9, mode)


def test_tile_skip_changes_no_value(harness, tmp_path):
    """a world with one cluster: most tiles of the box are filled without the sweeps, and the field equals the one with
    every tile live"""
    rng = np.random.default_rng(11)
    w = np.zeros((256, 256, 256), bool)
    w[100:120, 30:50, 200:220] = rng.random((20, 20, 20)) < 0.1
    origin, dims = (-10, 0, 60), (200, 130, 190)
    for radius, mode in [(9, R.TO_SOLID), (40, R.TO_SOLID), (9, R.TO_EMPTY)]:
        world = w if mode == R.TO_SOLID else ~w
        want = R.fast(world, origin, dims, radius, mode)
        on = _run_harness(harness, tmp_path, world, 32, origin, dims, radius, mode, skip=1)
        off = _run_harness(harness, tmp_path, world, 32, origin, dims, radius, mode, skip=0)
        assert off["live"] == off["tiles"] == 4 * 3 * 3 and 1 <= on["live"] < on["tiles"]
        for got in (on, off):
            assert np.array_equal(got["dist2"], want["dist2"]) and got["summary"] == want["summary"]
        assert want["summary"][1] > 1000 and want["summary"][2] > 1000


def _layout(harness, tmp_path, origin, dims, radius):
    raw, _ = run_harness_files(harness, tmp_path, [1, 8, 64, 64, 64, *origin, *dims, radius, 0, 1])
    with_o, without = (int(v) for v in np.frombuffer(raw[:8].tobytes(), np.uint32))
    return bool(with_o), bool(without), int(np.frombuffer(raw[8:16].tobytes(), np.uint64)[0])


def test_layout_accepts_the_last_origin_whose_halo_fits_int32(harness, tmp_path):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    for radius, dims in [(1, (8, 8, 8)), (255, (8, 3, 70)), (40, (1, 1, 1)), (2, (33, 2, 2))]:
        for k in range(3):
            for edge, ok in [(lo + radius, True), (lo + radius - 1, False), (hi - dims[k] - radius, True),
                             (hi - dims[k] - radius + 1, False)]:
                origin = [0, 0, 0]
                origin[k] = edge
                assert _layout(harness, tmp_path, origin, dims, radius)[:2] == (ok, True), (radius, dims, k, edge)


def _expect_bytes(d, radius):  # the formula of include/vxrt.h
    r = lambda n: (n + 255) // 256 * 256
    h = [v + 2 * radius for v in d]
    wh = (h[0] + 31) // 32
    T = [(v + 63) // 64 for v in d]
    return r(4 * wh * h[1] * h[2]) + r(2 * d[0] * d[1] * h[2]) + r(wh * ((h[1] + 7) // 8) * ((h[2] + 7) // 8)) + r(T[0] * T[1] * T[2])


def test_distance_symbols_exported_and_workspace_bytes(harness, tmp_path):
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_distance_workspace_bytes", "vxrt_distance_field", "vxrt_distance_field_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    ws = lambda d, r: int(lib.vxrt_distance_workspace_bytes((C.c_int32 * 3)(*d), r))
    for bad in [(0, 8, 8), (8, -1, 8), (1 << 10, 1 << 10, (1 << 8) + 1), (1 << 29, 1, 1)]:
        assert ws(bad, 4) == 0
    for bad in (0, 256, 1 << 31):
        assert ws((8, 8, 8), bad) == 0
    assert ws((1, 1, 1 << 28), 255) == 0 and ws((1, 1, 1 << 18), 255) > 0  # the halo box against 2^36 voxels
    assert lib.vxrt_distance_workspace_bytes(None, 4) == 0
    for d in [(1, 1, 1), (33, 7, 5), (256, 64, 256), (512, 256, 512), (1024, 256, 1024), (1, 1 << 14, 1 << 14)]:
        for radius in (1, 9, 32, 255):
            want = _expect_bytes(d, radius)
            if (d[0] + 2 * radius) * (d[1] + 2 * radius) * (d[2] + 2 * radius) > 1 << 36:
                want = 0
            assert ws(d, radius) == want, (d, radius)
            if d[0] <= 64:
                assert _layout(harness, tmp_path, (0, 0, 0), d, radius)[2] == want
    assert ws((512, 256, 512), 16) <= 2.5 * 512 * 256 * 512
    o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    assert lib.vxrt_distance_field(None, o3, d3, 4, 0, None, None, None, None) == -1
    assert lib.vxrt_distance_field_host(None, o3, d3, 4, 0, None, None) == -1
    assert (vx.DIST_TO_SOLID, vx.DIST_TO_EMPTY, vx.DIST_FAR, vx.DIST_MAX_RADIUS) == (0, 1, 0xFFFF, 255)
