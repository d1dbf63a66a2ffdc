"""CPU checks of floating-island detection (include/vxrt.h, vxrt_find_islands): the two restatements of tests/ref_islands.py
against each other and on hand-derived cases, and the kernels' island code (csrc/vxrt_islands.hpp) compiled for the host
(tests/tools/islands_check.cpp) against them -- labels, floating bits, table and summary bit-equal, every index checked."""
import ctypes as C

import numpy as np
import pytest

from tests import ref_islands as R
from tests.helpers import build_harness, run_harness_files

ALL = R.FACES | R.FLOOR


def _both(vox, origin=(0, 0, 0), anchors=ALL):
    """both restatements, asserted equal; returns the numpy one"""
    a = R.find_islands(vox, origin, anchors)
    if R.have_scipy():
        b = R.find_islands_scipy(vox, origin, anchors)
        assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["floating"], b["floating"])
        assert np.array_equal(a["table"], b["table"]) and a["summary"] == b["summary"]
    return a


@pytest.mark.parametrize("density", [0.05, 0.2, 0.31, 0.5])
def test_the_two_restatements_agree_on_random_grids(density):
    rng = np.random.default_rng(int(density * 100))
    vox = rng.random((37, 20, 26)) < density
    for origin, anchors in [((0, 0, 0), ALL), ((3, -5, 2), ALL), ((0, 0, 0), 0), ((1, -19, 0), R.FLOOR), ((0, 0, 0), R.X_HI | R.Z_LO)]:
        r = _both(vox, origin, anchors)
        assert r["summary"][0] > 0
        if anchors == 0:
            assert r["summary"][1] == r["summary"][0] and r["summary"][2] == int(vox.sum())


def _overhang():
    v = np.zeros((12, 12, 12), bool)
    v[:, 0, :] = True          # ground
    v[5, 1:8, 5] = True        # stem
    v[2:9, 8, 2:9] = True      # slab on top of the stem
    return v


def test_overhang_cut_from_its_stem():
    v = _overhang()
    r = _both(v, anchors=R.FLOOR)
    assert r["summary"] == (1, 0, 0)
    v[5, 4, 5] = False         # cut the stem: the upper stem and the slab fall
    r = _both(v, anchors=R.FLOOR)
    assert r["summary"] == (2, 1, 49 + 3)
    t = r["table"][0]
    assert t[0] == 1 + 2 + 12 * (8 + 12 * 2) and list(t[2:]) == [2, 5, 2, 9, 9, 9]
    assert r["floating"][5, 5:8, 5].all() and not r["floating"][:, 0, :].any()
    # the property: with the six faces of a box around the cut, the island is the same piece of the whole world
    b = R.find_islands(v[1:11, 1:11, 1:11], (1, 1, 1), R.FACES)
    assert b["summary"][1] == 1 and b["table"][0][1] == 52 and list(b["table"][0][2:]) == [2, 5, 2, 9, 9, 9]


def test_diagonal_contact_does_not_connect():
    v = np.zeros((6, 6, 6), bool)
    v[2, 2, 2] = v[3, 3, 2] = v[2, 3, 3] = v[3, 2, 3] = True  # edge contacts only
    v[4, 4, 4] = True                                          # a corner contact with (3, 3, 3)? no: (3, 3, 3) is empty
    r = _both(v, anchors=0)
    assert r["summary"] == (5, 5, 5)
    v[3, 3, 3] = True
    r = _both(v, anchors=0)
    assert r["summary"] == (3, 3, 6)  # (3,3,3) joins (3,3,2), (2,3,3), (3,2,3) by faces; (2,2,2), (4,4,4) only by corners


def test_ring_around_a_hole_is_one_component():
    v = np.zeros((9, 3, 9), bool)
    v[2:7, 1, 2:7] = True
    v[3:6, 1, 3:6] = False
    v[4, 1, 4] = True          # a voxel in the hole touches nothing
    r = _both(v, anchors=0)
    assert r["summary"] == (2, 2, 17)
    assert list(r["table"][:, 1]) == [16, 1]


def test_one_voxel_bridge_to_an_anchor_face():
    v = np.zeros((10, 10, 10), bool)
    v[4:7, 4:7, 4:7] = True
    v[0:4, 5, 5] = True        # a bridge of single voxels to the x-lo face
    r = _both(v, anchors=R.X_LO)
    assert r["summary"] == (1, 0, 0)
    v[2, 5, 5] = False
    r = _both(v, anchors=R.X_LO)
    assert r["summary"] == (2, 1, 27 + 1) and r["table"][0][1] == 28


def test_spiral_snake_is_one_component():
    v = R.snake((32, 32, 32))
    r = _both(v, anchors=0)
    assert r["summary"] == (1, 1, int(v.sum()))
    assert r["table"][0][0] == 1 and list(r["table"][0][2:]) == [0, 0, 0, 32, 31, 31]
    v2 = v.copy()
    v2[16, 0, 0] = False       # cut near the start: two pieces, the longer one's id is its first voxel
    r = _both(v2, anchors=0)
    assert r["summary"][0] == 2 and r["table"][1][0] == 1 + 17


def test_floor_bit_with_origin_below_zero():
    v = np.zeros((8, 12, 8), bool)
    v[3, 4:9, 3] = True        # a column standing on world y = 0 (box y = 4)
    v[6, 7, 6] = True
    r = _both(v, (10, -4, 10), R.FLOOR)
    assert r["summary"] == (2, 1, 1) and list(r["table"][0][2:]) == [16, 3, 16, 17, 4, 17]
    r = _both(v, (10, -3, 10), R.FLOOR)  # world y = 0 is box y = 3: the column's foot is above it, nothing anchors
    assert r["summary"] == (2, 2, 6)


def test_box_partly_outside_the_world():
    from oracle import ref_region
    world = np.zeros((16, 16, 16), bool)
    world[0:3, 0:16, 0:3] = True   # a pillar at the world's corner
    box = ref_region.read_region(world, (-4, -4, -4), (10, 24, 10))
    r = _both(box, (-4, -4, -4), R.FACES)
    assert r["summary"] == (1, 1, 3 * 16 * 3)  # the box faces lie outside the world: nothing anchors the pillar
    r = _both(box, (-4, -4, -4), ALL)
    assert r["summary"] == (1, 0, 0)


# ---- the kernels' island code on the host ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "islands_check")


def _run_harness(harness, tmp_path, world, factor, origin, dims, anchors, max_islands=1 << 20):
    from oracle import vxo
    X, Y, Z = world.shape
    raw, _ = run_harness_files(harness, tmp_path, [factor, X, Y, Z, *origin, *dims, anchors, max_islands],
                               vxo.dense_from_voxels(world))
    raw = raw.view(np.uint32)
    n = dims[0] * dims[1] * dims[2]
    wpr = (dims[0] + 31) // 32
    nb = wpr * dims[1] * dims[2]
    summary = tuple(int(v) for v in raw[:3])
    labels = raw[3:3 + n].reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)
    floating = raw[3 + n:3 + n + nb]
    table = raw[3 + n + nb:].view(np.int32).reshape(-1, 8).astype(np.int64)
    return summary, labels, floating, table


def _assert_harness(harness, tmp_path, world, factor, origin, dims, anchors, max_islands=1 << 20):
    from oracle import ref_region
    import voxelengine_amd as vx
    s, lab, fl, tab = _run_harness(harness, tmp_path, world, factor, origin, dims, anchors, max_islands)
    want = R.fast(ref_region.read_region(world, origin, dims), origin, anchors)
    assert s == want["summary"]
    assert np.array_equal(lab, want["labels"])
    assert np.array_equal(fl, vx.pack_region(want["floating"]))
    assert np.array_equal(tab, want["table"][:max_islands])
    return want


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    world = np.zeros((64, 64, 64), bool)
    v = _overhang()
    v[5, 4, 5] = False
    world[:12, :12, :12] = v
    world[20:52, 20:52, 20:52] = R.snake((32, 32, 32))
    for origin, dims, anchors in [((0, 0, 0), (12, 12, 12), R.FLOOR), ((1, 1, 1), (10, 10, 10), R.FACES),
                                  ((20, 20, 20), (32, 32, 32), 0), ((-3, -2, -5), (40, 30, 70), ALL)]:
        _assert_harness(harness, tmp_path, world, 8, origin, dims, anchors)


@pytest.mark.parametrize("factor,shape,density", [(8, (64, 64, 64), 0.31), (16, (128, 128, 128), 0.2),
                                                  (32, (256, 256, 256), 0.05), (8, (8192, 64, 64), 0.31)])
def test_host_code_equals_the_reference_on_random_worlds(harness, tmp_path, factor, shape, density):
    """boxes with dims not multiples of 32 or 16, half outside the world, every anchor mask that matters, a cut-short table"""
    rng = np.random.default_rng(factor + shape[0])
    world = rng.random(shape) < density
    boxes = [((0, 0, 0), shape, ALL), ((5, 3, 7), (45, 33, 17), R.FACES), ((-20, -10, -30), (61, 50, 70), ALL),
             ((shape[0] - 30, 2, 1), (47, 19, 40), 0), ((1, 0, 2), (1, 40, 33), R.Y_LO | R.Z_HI), ((7, 9, 3), (70, 1, 1), R.X_LO)]
    for origin, dims, anchors in boxes:
        dims = tuple(min(d, 96) for d in dims)
        want = _assert_harness(harness, tmp_path, world, factor, origin, dims, anchors)
        assert want["summary"][0] > 0
    _assert_harness(harness, tmp_path, world, factor, (3, 3, 3), (50, 40, 30), R.FACES, max_islands=5)


def test_islands_symbols_exported_and_workspace_bytes():
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_islands_workspace_bytes", "vxrt_find_islands", "vxrt_find_islands_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    ws = lambda d: int(lib.vxrt_islands_workspace_bytes((C.c_int32 * 3)(*d)))
    for bad in [(0, 8, 8), (8, -1, 8), (1 << 10, 1 << 10, (1 << 8) + 1), (1 << 29, 1, 1)]:
        assert ws(bad) == 0
    assert lib.vxrt_islands_workspace_bytes(None) == 0

    def expect(d):  # the layout of csrc/vxrt_islands.hpp: sections of words on 256-byte boundaries
        up = lambda w: (w + 63) // 64 * 64
        n = d[0] * d[1] * d[2]
        nw = (n + 63) // 64 * 2
        return 4 * (up((d[0] + 31) // 32 * d[1] * d[2]) + up(n) + 3 * up(nw) + up((nw + 1023) // 1024))
    for d in [(1, 1, 1), (33, 7, 5), (256, 256, 256), (512, 512, 512), (64, 64, 64), (1, 1 << 14, 1 << 14), (1 << 10, 1 << 10, 1 << 8)]:
        assert ws(d) == expect(d), d
        n = d[0] * d[1] * d[2]
        assert ws(d) <= 8.5 * n + 4096
        if d[0] >= 32:
            assert ws(d) <= 4.7 * n + 4096
    o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    assert lib.vxrt_find_islands(None, o3, d3, 0, None, None, None, None, 0, None, None) == -1
    assert lib.vxrt_find_islands_host(None, o3, d3, 0, None, None, None, 0, None) == -1
    assert vx.ISLAND_DTYPE.itemsize == 32 and vx.ISLAND_ANCHOR_FLOOR == 64 and vx.ISLAND_ANCHOR_FACES == 63
    isl = vx.Islands((0, 0, 0), (4, 4, 4), None, None,
                     np.asarray([[5, 2, 1, 2, 3, 2, 4, 4]], np.int32).view(vx.ISLAND_DTYPE).reshape(-1), vx.IslandSummary(1, 1, 2))
    b = isl.bodies((0, -1, 0))
    assert vx.Body.pack(b).tolist() == [[1, 2, 3, 2, 4, 4, 0, -1, 0]]
