"""Region readback and voxel stamps (include/vxrt.h, vxrt_read_region / vxrt_edit_stamps) without a GPU: the oracle's two
restatements (C: oracle/vxo_region.c; numpy: oracle/ref_region.py) on hand-derived cases and against each other, the
region word layout (voxelengine_amd.pack_region / unpack_region), the row logic of the library
(voxelengine_amd/csrc/vxrt_region.hpp) compiled for the host and held against the oracle, and the new ABI symbols."""

import numpy as np
import pytest

from tests.helpers import build_harness, run_harness

REPLACE, UNION, SUBTRACT = 0, 1, 2


def _read_both(vxo, vox, origin, dims):
    """the C restatement (dense tiled words -> region words) and the numpy one (bool grid); asserted equal"""
    import voxelengine_amd as vx
    from oracle import ref_region, vxo_region
    X, Y, Z = vox.shape
    words = vxo_region.read_region(vxo.dense_from_voxels(vox), X, Y, Z, origin, dims)
    p = ref_region.read_region(vox, origin, dims)
    assert np.array_equal(words, vx.pack_region(p))
    assert np.array_equal(vx.unpack_region(words, dims), p)
    return p, words


def _stamp_both(vxo, vox, stamps):
    """stamps: (origin, bool mask, mode); both restatements applied, asserted equal"""
    import voxelengine_amd as vx
    from oracle import ref_region, vxo_edit, vxo_region
    X, Y, Z = vox.shape
    cs = [(o, vx.pack_region(m), m.shape, mode) for o, m, mode in stamps]
    c = vxo_edit.voxels_from_dense(vxo_region.apply_stamps(vxo.dense_from_voxels(vox), X, Y, Z, cs), X, Y, Z)
    p = ref_region.apply_stamps(vox, stamps)
    assert np.array_equal(c, p)
    return p


def test_pack_unpack_round_trip_and_layout():
    import voxelengine_amd as vx
    rng = np.random.default_rng(2)
    for dims in [(1, 1, 1), (1, 5, 3), (31, 2, 2), (32, 3, 1), (33, 2, 3), (65, 4, 2), (100, 1, 7)]:
        v = rng.random(dims) < 0.5
        w = vx.pack_region(v)
        wpr = (dims[0] + 31) // 32
        assert w.dtype == np.uint32 and w.size == wpr * dims[1] * dims[2] == vx.region_words(dims)
        assert np.array_equal(vx.unpack_region(w, dims), v)
        for x, y, z in zip(*np.nonzero(v)):           # voxel (x, y, z): bit x & 31 of word (y + Y z) wpr + x >> 5
            assert (int(w[(y + dims[1] * z) * wpr + (x >> 5)]) >> (x & 31)) & 1
        assert int(np.unpackbits(w.view(np.uint8), bitorder="little").sum()) == int(v.sum())   # padding bits 0
    assert vx.region_words((0, 4, 4)) == 0 and vx.region_words((4, -1, 4)) == 0
    assert vx.region_words((1 << 12, 1 << 12, 1 << 12)) == 1 << 31 and vx.region_words((1 << 12, 1 << 12, 4097)) == 0


def test_reads_crossing_every_face_and_outside(vxo):
    rng = np.random.default_rng(3)
    vox = rng.random((32, 24, 40)) < 0.4
    p, _ = _read_both(vxo, vox, (-3, -5, -7), (40, 30, 50))       # crosses all six faces
    assert np.array_equal(p[3:35, 5:29, 7:47], vox) and not p[:3].any() and not p[35:].any()
    assert not p[:, :5].any() and not p[:, 29:].any() and not p[:, :, :7].any() and not p[:, :, 47:].any()
    for origin in [(32, 0, 0), (0, 24, 0), (0, 0, 40), (-10, 0, 0), (0, -7, 5), (2147483600, 0, 0), (-2147483648, 0, 0)]:
        p, w = _read_both(vxo, vox, origin, (10, 7, 5))              # wholly outside: zeros
        assert not p.any() and not w.any()
    p, _ = _read_both(vxo, vox, (5, 6, 7), (1, 1, 1))              # a single voxel
    assert p.shape == (1, 1, 1) and p[0, 0, 0] == vox[5, 6, 7]


@pytest.mark.parametrize("d0", [1, 31, 32, 33, 65])
def test_read_row_widths_and_zero_padding(vxo, d0):
    vox = np.ones((96, 16, 16), bool)
    p, w = _read_both(vxo, vox, (3, 2, 1), (d0, 5, 4))
    assert p.all()
    wpr = (d0 + 31) // 32
    last = w.reshape(4, 5, wpr)[:, :, -1]
    assert np.all(last == np.uint32((1 << (d0 - 32 * (wpr - 1))) - 1 if d0 % 32 else 0xFFFFFFFF))


def test_stamp_modes_on_hand_derived_cases(vxo):
    vox = np.zeros((16, 16, 16), bool)
    vox[0:8] = True                                                  # x < 8 solid
    m = np.zeros((4, 4, 4), bool)
    m[0:2] = True                                                    # the stamp's x 0, 1 set, x 2, 3 clear
    o = (6, 3, 3)                                                    # stamp x 6..9: 6, 7 solid and 8, 9 empty in the world
    rep = _stamp_both(vxo, vox, [(o, m, REPLACE)])
    uni = _stamp_both(vxo, vox, [(o, m, UNION)])
    sub = _stamp_both(vxo, vox, [(o, m, SUBTRACT)])
    box = (slice(6, 10), slice(3, 7), slice(3, 7))
    assert np.array_equal(rep[box], m)                               # replace: the box becomes the mask
    assert np.array_equal(uni[box], m | vox[box])                    # union: m = 1 sets, m = 0 keeps
    assert np.array_equal(sub[box], vox[box] & ~m)                   # subtract: m = 1 clears, m = 0 keeps
    outside = np.ones_like(vox)
    outside[box] = False
    for r in (rep, uni, sub):
        assert np.array_equal(r[outside], vox[outside])


def test_last_stamp_wins(vxo):
    vox = np.zeros((16, 16, 16), bool)
    full = np.ones((6, 6, 6), bool)
    hole = np.zeros((6, 6, 6), bool)
    # replace after union: the replace decides the whole overlap
    r = _stamp_both(vxo, vox, [((2, 2, 2), full, UNION), ((4, 4, 4), hole, REPLACE)])
    assert not r[4:10, 4:10, 4:10].any() and r[2:4, 2:8, 2:8].all()
    # union after subtract: the union sets what the subtract cleared
    r = _stamp_both(vxo, np.ones_like(vox), [((0, 0, 0), full, SUBTRACT), ((3, 3, 3), full, UNION)])
    assert r[3:9, 3:9, 3:9].all() and not r[0:3, 0:3, 0:3].any()
    # subtract after replace
    r = _stamp_both(vxo, vox, [((0, 0, 0), full, REPLACE), ((1, 1, 1), full, SUBTRACT)])
    assert r.sum() == 6 ** 3 - 5 ** 3


def test_stamps_clipped_to_the_world(vxo):
    rng = np.random.default_rng(4)
    vox = rng.random((16, 16, 16)) < 0.3
    m = rng.random((20, 20, 20)) < 0.5
    r = _stamp_both(vxo, vox, [((-10, -3, 5), m, REPLACE)])
    assert np.array_equal(r[0:10, 0:16, 5:16], m[10:20, 3:19, 0:11])
    assert np.array_equal(r[10:], vox[10:]) and np.array_equal(r[:, :, :5], vox[:, :, :5])
    for o in [(16, 0, 0), (0, -20, 0), (2147483000, 0, 0)]:
        assert np.array_equal(_stamp_both(vxo, vox, [(o, m, REPLACE)]), vox)


def test_invalid_stamps_are_refused(vxo):
    from oracle import ref_region, vxo_region
    vox = np.zeros((8, 8, 8), bool)
    dense = vxo.dense_from_voxels(vox)
    ok = ((0, 0, 0), np.ones(1, np.uint32), (1, 1, 1), REPLACE)
    for bad in [((0, 0, 0), np.ones(1, np.uint32), (1, 1, 1), 3), ((0, 0, 0), np.ones(1, np.uint32), (0, 1, 1), UNION),
                ((0, 0, 0), None, (1, 1, 1), UNION), ((0, 0, 0), np.ones(1, np.uint32), (1 << 12, 1 << 12, 4097), UNION)]:
        with pytest.raises(ValueError):
            vxo_region.apply_stamps(dense, 8, 8, 8, [ok, bad])
    with pytest.raises(ValueError):
        ref_region.apply_stamps(vox, [((0, 0, 0), np.ones((1, 1, 1), bool), REPLACE), ((0, 0, 0), np.ones((1, 1, 1), bool), 7)])
    with pytest.raises(ValueError):
        vxo_region.read_region(dense, 8, 8, 8, (0, 0, 0), (1, 0, 1))


def test_c_and_numpy_restatements_agree(vxo):
    rng = np.random.default_rng(11)
    S = 48
    for i in range(300):
        vox = rng.random((S, S, S)) < (0.0 if i % 4 == 0 else 0.2)
        stamps = []
        for _ in range(int(rng.integers(0, 6))):
            dims = tuple(int(rng.integers(1, 40)) for _ in range(3))
            origin = tuple(int(rng.integers(-30, S + 5)) for _ in range(3))
            stamps.append((origin, rng.random(dims) < rng.random(), int(rng.integers(0, 3))))
        out = _stamp_both(vxo, vox, stamps)
        dims = tuple(int(rng.integers(1, 70)) for _ in range(3))
        origin = tuple(int(rng.integers(-30, S + 5)) for _ in range(3))
        _read_both(vxo, out, origin, dims)


def test_copy_paste_and_undo_on_the_oracle(vxo):
    """the recipes of INTEGRATION.md on the numpy restatement: copy + paste, and read / edit / replace-stamp = undo"""
    from oracle import ref_edit, ref_region
    rng = np.random.default_rng(6)
    vox = rng.random((64, 64, 64)) < 0.3
    clip = ref_region.read_region(vox, (5, 6, 7), (20, 10, 30))
    pasted = ref_region.apply_stamps(vox, [((30, 40, 20), clip, REPLACE)])
    assert np.array_equal(pasted[30:50, 40:50, 20:50], vox[5:25, 6:16, 7:37])
    before = ref_region.read_region(vox, (10, 10, 10), (30, 30, 30))
    edited = ref_edit.apply_edits(vox, [(1, 0, (25, 25, 25), (10, 0, 0)), (0, 1, (12, 12, 12), (20, 30, 22))])
    assert not np.array_equal(edited, vox)
    assert np.array_equal(ref_region.apply_stamps(edited, [((10, 10, 10), before, REPLACE)]), vox)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "region_check", "vxo_region.c")


def test_host_row_helpers_and_validation(harness):
    """row gather, funnel placement, coverage masks, region_words and stamp validation / clipping on hand-derived cases"""
    run_harness(harness, "units")


@pytest.mark.parametrize("factor,X,Y,Z,rounds", [(8, 64, 64, 64, 6), (16, 128, 128, 128, 3), (32, 256, 256, 256, 2),
                                                 (8, 8192, 64, 64, 1)])
def test_host_read_logic_equals_the_oracle(harness, factor, X, Y, Z, rounds):
    """k_read_region's word (clipping, the bricks a word crosses, funnel shifts, padding) for random boxes, including
    boxes across every face, wholly outside and a single voxel, on random worlds; the last case is a wide grid"""
    out = run_harness(harness, "read", factor, X, Y, Z, rounds)
    assert int(out.split(" voxels set")[0].split()[-1]) > 0


@pytest.mark.parametrize("factor,X,Y,Z,rounds", [(8, 64, 64, 64, 9), (16, 128, 128, 128, 3), (32, 256, 256, 256, 3),
                                                 (8, 8192, 64, 64, 1)])
def test_host_stamp_logic_equals_the_oracle(harness, factor, X, Y, Z, rounds):
    """k_stamp_bricks' functions (filter from the last covering replace stamp, row gather, coverage, the three modes,
    extents from the rows) brick by brick: images and packed extents equal the oracle's rebuilt brickmap of the stamped
    dense grid, for every brick of random worlds"""
    out = run_harness(harness, "stamp", factor, X, Y, Z, rounds)
    assert int(out.split(" changed")[0].split()[-1]) > 0


def test_region_symbols_exported():
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_region_words", "vxrt_read_region", "vxrt_read_region_host", "vxrt_edit_stamps"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    assert lib.vxrt_abi_version() == 3
    # no context: refused before anything else
    import ctypes as C
    d = (C.c_int32 * 3)(4, 4, 4)
    assert lib.vxrt_read_region(None, d, d, None, None) == -1
    assert lib.vxrt_read_region_host(None, d, d, None) == -1
    assert lib.vxrt_edit_stamps(None, None, 0, None) == -1
    assert lib.vxrt_region_words(d) == 4 * 4
    assert C.sizeof(vx.StampDesc) == 40
