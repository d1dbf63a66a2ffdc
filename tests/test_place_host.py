"""CPU checks of the voxel piece queries (include/vxrt.h, vxrt_place_pieces): the two restatements of tests/ref_place.py
against each other on the hand-derived cases of tests/place_cases.py and on random inputs, the falling-island rule on its
cases, and the kernels' per-lane code (csrc/vxrt_place.hpp) compiled for the host (tests/tools/place_check.cpp) against the
restatements, bit for bit, at several launch shapes, with every index it forms checked."""
import ctypes as C

import numpy as np
import pytest

from tests import place_cases as PC
from tests import ref_place as R
from tests.helpers import build_harness, run_harness_files


def _pack(vox):
    import voxelengine_amd as vx
    return vx.pack_region(vox)


def _both(vox, pieces, placements):
    a, b = R.place(vox, pieces, placements, R.place_shift), R.place(vox, pieces, placements, R.place_clearance)
    assert np.array_equal(a, b), np.flatnonzero((a != b).any(1))[:10]
    return a


def random_pieces(rng):
    shapes = [((1, 1, 1), 1.0), ((9, 5, 7), 0.3), ((31, 3, 2), 0.5), ((32, 3, 2), 0.5), ((33, 4, 3), 0.5), ((64, 2, 2), 0.5),
              ((65, 3, 2), 0.5), ((3, 40, 33), 0.2), ((5, 5, 5), 0.0), ((33, 2, 1), 0.5)]
    return [rng.random(s) < d for s, d in shapes]


def random_world(rng, dims, density=0.002):
    v = rng.random(dims, dtype=np.float32) < density
    v[:, : dims[1] // 4, :] |= rng.random((dims[0], dims[1] // 4, dims[2]), dtype=np.float32) < 0.5  # a rough ground
    return v


def random_placements(rng, dims, n, n_pieces, dmax=12):
    pl = np.zeros((n, 6), np.int32)
    pl[:, 0] = rng.integers(0, n_pieces, n)
    for k in range(3):
        pl[:, 1 + k] = rng.integers(-8, dims[k], n)
    pl[:, 4] = rng.integers(0, 3, n)
    pl[:, 5] = rng.integers(-dmax, dmax + 1, n)
    return pl


def classes(want):
    """shares of: free over the whole distance, blocked after moving, blocked at the first step, overlapping at the start"""
    blocked = (want[:, 3] & R.BLOCKED) != 0
    n = float(len(want))
    return (np.count_nonzero(~blocked) / n, np.count_nonzero(blocked & (want[:, 1] != 0)) / n,
            np.count_nonzero(blocked & (want[:, 1] == 0)) / n, np.count_nonzero(want[:, 0] > 0) / n)


@pytest.mark.parametrize("case", PC.CASES, ids=[c[0] for c in PC.CASES])
def test_hand_derived_cases(case):
    _, vox, piece, origin, axis, dist, want = case
    got = _both(vox, [piece], [[0, *origin, axis, dist]])
    assert tuple(got[0]) == want


@pytest.mark.parametrize("seed", range(3))
def test_the_two_restatements_agree_on_random_cases(seed):
    rng = np.random.default_rng(300 + seed)
    dims = [(24, 32, 24), (40, 24, 16), (16, 48, 33)][seed]
    vox = random_world(rng, dims, 0.01)
    pieces = random_pieces(rng)
    pl = random_placements(rng, dims, 400, len(pieces))
    pl[::50, 0] = len(pieces)  # invalid ones among them
    want = _both(vox, pieces, pl)
    assert np.count_nonzero(want[:, 3] == R.INVALID) == 8 and min(classes(want)) > 0.05


def test_validity_rule():
    ok = [0, 1, 2, 3, 1, -4]
    cases = [(ok, True), ([1, 1, 2, 3, 1, -4], False), ([-1, 1, 2, 3, 1, -4], False), ([0, 1, 2, 3, 3, 1], False),
             ([0, 1, 2, 3, -1, 1], False), ([0, 1, 2, 3, 0, 4096], True), ([0, 1, 2, 3, 0, -4096], True),
             ([0, 1, 2, 3, 0, 4097], False), ([0, 1, 2, 3, 2, -4097], False), ([0, 1 << 30, -(1 << 30), 0, 2, 0], True),
             ([0, (1 << 30) + 1, 0, 0, 2, 0], False), ([0, 0, -(1 << 30) - 1, 0, 2, 0], False), ([0, 0, 0, (1 << 30) + 1, 2, 0], False)]
    for pl, good in cases:
        assert R.valid(pl, 1) == good, pl
    got = R.place(PC.floor_world(), [PC.cube()], [c[0] for c in cases])
    for row, (_, good) in zip(got, cases):
        assert (tuple(row) == (0, 0, 0, R.INVALID)) == (not good)


@pytest.mark.parametrize("case", PC.DROP_CASES, ids=[c[0] for c in PC.DROP_CASES])
def test_drop_rule_on_its_cases(case):
    _, vox, origin, dims, want_rows = case
    for how in (R.place_shift, R.place_clearance):
        after, rows = R.drop_islands(vox, origin, dims, how=how)
        assert rows.tolist() == [list(r) for r in want_rows]
        assert after.sum() == vox.sum()  # the voxels are conserved
        again, rows2 = R.drop_islands(after, origin, dims)
        assert len(rows2) == 0 and np.array_equal(again, after)  # everything has landed: nothing floats any more
    if case[0] == "two stacked cubes":
        assert after[4:6, 2:6, 4:6].all() and after[:, 6:, :].sum() == 0  # A on the floor, B on A
    with pytest.raises(ValueError):
        R.drop_islands(vox, origin, dims, max_islands=0)


# ---- the kernels' per-lane code on the host ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "place_check")


def _run_harness(harness, tmp_path, vox, factor, piece_words, piece_dims, placements, lanes=0):
    from oracle import vxo
    X, Y, Z = vox.shape
    pl = np.ascontiguousarray(placements, np.int32).reshape(-1, 6)
    arrays = [vxo.dense_from_voxels(vox)]
    for w, d in zip(piece_words, piece_dims):
        arrays += [np.asarray(d, np.int32), np.asarray(w, np.uint32)]
    raw, stdout = run_harness_files(harness, tmp_path, [factor, X, Y, Z, len(pl), len(piece_words), lanes], *arrays, pl)
    return raw.view(np.uint32).reshape(-1, 4), stdout


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    for _, small, piece, origin, axis, dist, want in PC.CASES:
        vox = np.zeros((64, 64, 64), bool)  # the case's world in a corner of one the brickmap builder takes at f = 8
        vox[:16, :16, :16] = small
        want = _both(vox, [piece], [[0, *origin, axis, dist]])  # (the larger world changes "out of the world" cases only)
        for words in (_pack(piece), PC.padded_words(piece)):  # set padding bits change nothing
            for lanes in (0, 1, 64):
                got, _ = _run_harness(harness, tmp_path, vox, 8, [words], [piece.shape], [[0, *origin, axis, dist]], lanes)
                assert np.array_equal(got, R.pack_results(want)), (_, lanes)


@pytest.mark.parametrize("factor,dims,lanes", [(8, (64, 64, 64), 0), (16, (128, 128, 128), 4), (32, (256, 256, 256), 1),
                                               (8, (64, 64, 64), 16)])
def test_host_code_equals_the_restatements_on_random_worlds(harness, tmp_path, factor, dims, lanes):
    """every piece shape of the GPU tests, placements half outside the world, every axis and direction, invalid ones included,
    at the library's launch shape and at others: bit-equal to the restatement, every index inside its array"""
    rng = np.random.default_rng(factor * 10 + lanes)
    vox = random_world(rng, dims)
    pieces = random_pieces(rng)
    words = [_pack(p) for p in pieces]
    words[-1] = PC.padded_words(pieces[-1])
    n = 600
    pl = random_placements(rng, dims, n, len(pieces))
    pl[::97, 4] = 3
    pl[5::97, 5] = 5000
    want = R.place(vox, pieces, pl)
    got, out = _run_harness(harness, tmp_path, vox, factor, words, [p.shape for p in pieces], pl, lanes)
    bad = np.flatnonzero((got != R.pack_results(want)).any(1))
    assert len(bad) == 0, (bad[:10], got[bad[:3]], want[bad[:3]], pl[bad[:3]])
    assert min(classes(want)) >= 0.1, classes(want)
    if lanes == 0:
        assert "lanes 64, tasks 21" in out  # 3 x 40 x 33: 1320 rows


def test_host_code_at_every_x_alignment(harness, tmp_path):
    rng = np.random.default_rng(5)
    vox = random_world(rng, (64, 64, 64), 0.02)
    piece = rng.random((33, 2, 2)) < 0.5
    pl = [[0, x, int(rng.integers(0, 60)), int(rng.integers(0, 60)), 0, d] for x in range(-40, 73) for d in (-40, 40)]
    want = _both(vox, [piece], pl)
    got, _ = _run_harness(harness, tmp_path, vox, 8, [_pack(piece)], [piece.shape], pl)
    assert np.array_equal(got, R.pack_results(want))
    assert np.count_nonzero(want[:, 3]) > 20 and np.count_nonzero(want[:, 3] == 0) > 20


def test_host_code_at_the_distance_limit(harness, tmp_path):
    vox = np.zeros((64, 4160, 64), bool)  # the smallest world of whole 8-cell tiles at f = 8 that is taller than the limit
    vox[3, 4100, 3] = True
    one = np.ones((1, 1, 1), bool)
    pl = [[0, 3, 4, 3, 1, 4096], [0, 3, 4, 3, 1, 4095], [0, 3, 4, 3, 1, -4096], [0, 3, 4, 3, 1, 4097], [0, 3, 4, 3, 1, -4097]]
    want = R.place(vox, [one], pl)
    assert want.tolist() == [[0, 4095, 1, 1], [0, 4095, 0, 0], [0, -4096, 0, 0], [0, 0, 0, 2], [0, 0, 0, 2]]
    got, _ = _run_harness(harness, tmp_path, vox, 8, [_pack(one)], [one.shape], pl)
    assert np.array_equal(got, R.pack_results(want))


def test_host_code_with_a_piece_of_many_tasks(harness, tmp_path):
    """a 64 x 48 x 40 piece (1920 rows: 30 tasks of 64 lanes) dropped onto a floor, swept along x and fitted"""
    rng = np.random.default_rng(9)
    vox = random_world(rng, (256, 256, 256), 0.001)
    piece = rng.random((64, 48, 40)) < 0.01
    piece[63, 47, 39] = True
    pl = [[0, 10, 40, 20, 1, -30], [0, 10, 40, 20, 0, 25], [0, 10, 10, 20, 2, 0], [0, 10, 40, 20, 2, -30]]
    want = _both(vox, [piece], pl)
    got, out = _run_harness(harness, tmp_path, vox, 32, [_pack(piece)], [piece.shape], pl)
    assert np.array_equal(got, R.pack_results(want)) and "tasks 30" in out
    assert want[0, 3] == R.BLOCKED and want[2, 0] > 0


def test_place_symbols_exported():
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_place_pieces", "vxrt_place_pieces_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    assert lib.vxrt_place_pieces(None, None, 1, None, 1, None, None) == -1  # a NULL ctx comes first
    assert lib.vxrt_place_pieces_host(None, None, 1, None, 1, None) == -1
    assert C.sizeof(vx.PieceDesc) == 24 and vx.PLACED_DTYPE.itemsize == 16
    assert (vx.PLACE_MAX_PIECES, vx.PLACE_MAX_DIM, vx.PLACE_MAX_VOXELS, vx.PLACE_MAX_DIST) == (64, 1024, 1 << 24, 4096)
    assert (vx.PLACED_BLOCKED, vx.PLACED_INVALID) == (1, 2)
    assert tuple(vx.Placement(0, (1, 2, 3))) == (0, (1, 2, 3), 1, 0)
