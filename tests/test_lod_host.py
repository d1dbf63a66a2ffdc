"""CPU checks of the occupancy LOD (include/vxrt.h, vxrt_downsample_region): the three restatements of tests/ref_lod.py
against each other, the invariants of the definition (monotone bits, ANY = OR and ALL = AND of the children, the pyramid of
counts, composition of ANY and of ALL, the solid total), hand-derived cases with their packed words written out, and the
kernels' per-lane code (csrc/vxrt_lod.hpp) compiled for the host (tests/tools/lod_check.cpp) against the restatements --
bits, counts and summary bit-equal, every index checked -- with the workspace formula and the limits of the shift, the
threshold, the source box and the origin."""
import numpy as np
import pytest

from tests import ref_lod as R
from tests.helpers import build_harness, run_harness_files

SHIFTS = (1, 2, 3, 4, 5)
# random cases: (world shape, density, origin, dims in cells at shift 1; halved per shift, at least (2, 1, 1)): boxes inside,
# partly outside and wholly outside the world, unaligned and negative origins
CASES = [((64, 64, 64), 0.01, (0, 0, 0), (32, 32, 32)), ((64, 64, 64), 0.2, (3, 1, 2), (24, 16, 20)), ((64, 64, 64), 0.5, (-3, -2, -1), (34, 14, 18)),
         ((64, 64, 64), 0.85, (37, 41, 39), (24, 18, 20)), ((64, 64, 64), 1.0, (-5, 30, 50), (40, 24, 28)), ((64, 64, 64), 0.5, (70, 0, 0), (8, 8, 8)),
         ((64, 64, 64), 0.6, (-90, -9, -9), (5, 5, 5)), ((128, 64, 64), 0.9, (1, -7, 2), (66, 6, 10)), ((64, 64, 64), 0.5, (63, 63, 63), (1, 1, 1)),
         ((64, 64, 64), 1.0, (-1, -1, -1), (33, 33, 33))]


def _dims(dims, shift):
    return tuple(max(d >> (shift - 1), 2 if k == 0 else 1) for k, d in enumerate(dims))


def _worlds():
    rng = np.random.default_rng(14)
    return [(rng.random(shape) < density, origin, dims) for shape, density, origin, dims in CASES]


def _thresholds(shift):
    full = 1 << (3 * shift)
    return sorted({1, 2, max(full // 2, 1), full - 1, full} - {0})


def _both(world, origin, dims, shift):
    a = R.counts_reshape(world, origin, dims, shift)
    assert np.array_equal(a, R.counts_prefix(world, origin, dims, shift))
    return a


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_restatements_agree_on_random_grids(shift):
    for world, origin, dims in _worlds():
        _both(world, origin, _dims(dims, shift), shift)


def test_the_loop_agrees_on_tiny_boxes():
    rng = np.random.default_rng(3)
    world = rng.random((16, 16, 16)) < 0.6
    for shift, origin, dims in [(1, (-1, 3, 13), (3, 2, 3)), (2, (5, -2, 9), (2, 2, 2)), (3, (-3, 11, 1), (2, 1, 2)), (4, (-7, 2, 5), (2, 1, 1)),
                                (5, (-20, -3, 1), (1, 1, 1))]:
        assert np.array_equal(R.counts_brute(world, origin, dims, shift), _both(world, origin, dims, shift))


@pytest.mark.parametrize("shift", SHIFTS)
def test_invariants_of_the_definition(shift):
    f = 1 << shift
    for world, origin, dims in _worlds():
        dims = _dims(dims, shift)
        c = _both(world, origin, dims, shift)
        src = R.source_box(world, origin, dims, shift)
        kids = src.reshape(dims[0], f, dims[1], f, dims[2], f)
        last = None
        for t in _thresholds(shift):  # bits are monotone in the threshold
            got = R.downsample(world, origin, dims, shift, t, c)
            assert last is None or not (got.bits & ~last).any()
            last = got.bits
            assert int(got.summary[0]) | int(got.summary[1]) << 32 == int(src.sum())  # solid: the voxels of the source box
            assert int(got.summary[3]) + int(got.summary[4]) + int(got.summary[5]) == c.size and got.summary[7] == 0
        assert np.array_equal(R.downsample(world, origin, dims, shift, 1, c).bits, kids.any(axis=(1, 3, 5)))  # ANY: the OR
        assert np.array_equal(R.downsample(world, origin, dims, shift, f ** 3, c).bits, kids.all(axis=(1, 3, 5)))  # ALL: the AND


def test_pyramid_consistency_and_composition():
    """counts at shift a + b are the 2^b-block sums of counts at shift a; down(down(w, a, ANY), b, ANY) == down(w, a + b, ANY),
    and the same for ALL"""
    for world, origin, _ in _worlds()[:8]:
        for a in (1, 2, 3, 4):
            for b in range(1, 6 - a):
                dims = (3, 2, 2)
                fine = tuple(d << b for d in dims)
                ca, cab = _both(world, origin, fine, a), _both(world, origin, dims, a + b)
                g = 1 << b
                assert np.array_equal(ca.reshape(dims[0], g, dims[1], g, dims[2], g).sum(axis=(1, 3, 5)), cab)
                for t_a, t_b, t_ab in [(1, 1, 1), (1 << 3 * a, 1 << 3 * b, 1 << 3 * (a + b))]:
                    mid = R.downsample(world, origin, fine, a, t_a, ca).bits  # a world of its own, origin 0
                    assert np.array_equal(R.downsample(mid, (0, 0, 0), dims, b, t_b).bits,
                                          R.downsample(world, origin, dims, a + b, t_ab, cab).bits)


# ---- hand-derived cases ---------------------------------------------------------------------------------------------------
def _corner_world(shift):
    """one voxel at each corner of cell (1, 0, 0) of a box at origin (1, 2, 3); cell (0, 0, 0) stays empty"""
    f = 1 << shift
    w = np.zeros((128, 64, 64), bool)
    for dx in (0, f - 1):
        for dy in (0, f - 1):
            for dz in (0, f - 1):
                w[1 + f + dx, 2 + dy, 3 + dz] = True
    return w


@pytest.mark.parametrize("shift", SHIFTS)
def test_hand_one_voxel_at_each_corner_of_a_cell(shift):
    got = R.downsample(_corner_world(shift), (1, 2, 3), (3, 1, 1), shift, 8)
    assert got.flat.tolist() == [0, 8, 0] and got.words.tolist() == [0b010]
    assert got.summary.tolist() == [8, 0, 1, 2, 1 if shift == 1 else 0, 0 if shift == 1 else 1, 8, 0]


def _full_cell_world(shift, missing):
    f = 1 << shift
    w = np.zeros((64, 64, 64), bool)
    w[f:2 * f, 0:f, 0:f] = True
    if missing:
        w[2 * f - 1, f - 1, f - 1] = False
    return w


@pytest.mark.parametrize("shift", SHIFTS)
def test_hand_full_cell_and_one_voxel_short_of_it(shift):
    full = 1 << (3 * shift)
    got = R.downsample(_full_cell_world(shift, False), (0, 0, 0), (2, 1, 1), shift, full)
    assert got.flat.tolist() == [0, full] and got.words.tolist() == [0b10] and got.summary.tolist() == [full, 0, 1, 1, 1, 0, full, 0]
    got = R.downsample(_full_cell_world(shift, True), (0, 0, 0), (2, 1, 1), shift, full)
    assert got.flat.tolist() == [0, full - 1] and got.words.tolist() == [0] and got.summary.tolist() == [full - 1, 0, 0, 1, 0, 1, full - 1, 0]
    assert R.downsample(_full_cell_world(shift, True), (0, 0, 0), (2, 1, 1), shift, full - 1).words.tolist() == [0b10]


@pytest.mark.parametrize("shift", SHIFTS)
def test_hand_cell_straddling_the_far_face(shift):
    """a solid world of 64^3 and a row of three cells whose middle one straddles x = 64 by one voxel slab"""
    f = 1 << shift
    got = R.downsample(np.ones((64, 64, 64), bool), (65 - 2 * f, 0, 0), (3, 1, 1), shift, f * f)
    assert got.flat.tolist() == [f ** 3, f * f * (f - 1), 0]
    assert got.words.tolist() == [0b011] and R.downsample(np.ones((64, 64, 64), bool), (65 - 2 * f, 0, 0), (3, 1, 1), shift,
                                                           f * f * (f - 1) + 1).words.tolist() == [0b001]


def _stripe_world():
    w = np.zeros((128, 64, 64), bool)
    w[::3, 0, 0] = True  # voxels x = 0, 3, 6, ...: a cell of f = 2 at X holds one exactly when X % 3 != 2
    return w


@pytest.mark.parametrize("nx", [1, 31, 32, 33])
def test_hand_padding_bits_are_zero(nx):
    got = R.downsample(_stripe_world(), (0, 0, 0), (nx, 1, 1), 1, 1)
    want = sum(1 << x for x in range(nx) if x % 3 != 2)
    assert got.words.tolist() == ([want] if nx <= 32 else [want & 0xFFFFFFFF, want >> 32])
    assert want >> nx == 0 and len(got.flat) == nx


# ---- the kernels' code on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "lod_check")


def _run_harness(harness, tmp_path, world, origin, dims, shift, threshold, counts=True, split=True, factor=8):
    from oracle import vxo
    X, Y, Z = world.shape
    header = [0, factor, X, Y, Z, *origin, *dims, shift, threshold, int(counts), int(split)]
    raw, _ = run_harness_files(harness, tmp_path, header, vxo.dense_from_voxels(world))
    nw = -(-dims[0] // 32) * dims[1] * dims[2]
    summary = np.frombuffer(raw[:32].tobytes(), np.uint32)
    words = np.frombuffer(raw[32:32 + 4 * nw].tobytes(), np.uint32)
    flat = np.frombuffer(raw[32 + 4 * nw:].tobytes(), np.uint16)
    assert len(flat) == (dims[0] * dims[1] * dims[2] if counts else 0)
    return summary, words, flat


def _assert_harness(harness, tmp_path, world, origin, dims, shift, threshold, **kw):
    want = R.downsample(world, origin, dims, shift, threshold, R.counts_reshape(world, origin, dims, shift))
    summary, words, flat = _run_harness(harness, tmp_path, world, origin, dims, shift, threshold, **kw)
    assert np.array_equal(summary, want.summary), (summary, want.summary)
    assert np.array_equal(words, want.words)
    if kw.get("counts", True):
        assert np.array_equal(flat, want.flat)
    return want


@pytest.mark.parametrize("shift", SHIFTS)
def test_harness_equals_the_restatements_on_random_grids(harness, tmp_path, shift):
    for i, (world, origin, dims) in enumerate(_worlds()):
        t = _thresholds(shift)
        _assert_harness(harness, tmp_path, world, origin, _dims(dims, shift), shift, t[i % len(t)], counts=i % 3 != 2, split=i % 2 == 0)


@pytest.mark.parametrize("shift", SHIFTS)
def test_harness_runs_across_output_words_and_waves(harness, tmp_path, shift):
    """output widths around a word and around a wave of lanes; density 0.85 so that fields carry between the SWAR stages"""
    rng = np.random.default_rng(22)
    world = rng.random((128, 64, 64)) < 0.85
    for nx in (1, 31, 32, 33, 64, 65):
        _assert_harness(harness, tmp_path, world, (-1, 3, -2), (nx, 3, 2), shift, _thresholds(shift)[2])


@pytest.mark.parametrize("shift,nxs", [(1, (1008, 1024, 1040)), (5, (63, 64, 65))])
def test_harness_runs_across_a_wave_of_source_words(harness, tmp_path, shift, nxs):
    """source rows of 63, 64 and 65 words on a world 2112 voxels long, two cells along y and z"""
    rng = np.random.default_rng(23)
    world = rng.random((2112, 64, 64)) < 0.5
    for nx in nxs:
        _assert_harness(harness, tmp_path, world, (17, 0, 0), (nx, 2, 2), shift, 1 << (3 * shift - 1))


@pytest.mark.parametrize("shift", SHIFTS)
def test_harness_on_the_hand_derived_worlds(harness, tmp_path, shift):
    full, f = 1 << (3 * shift), 1 << shift
    assert _assert_harness(harness, tmp_path, _corner_world(shift), (1, 2, 3), (3, 1, 1), shift, 8).words.tolist() == [0b010]
    assert _assert_harness(harness, tmp_path, _full_cell_world(shift, False), (0, 0, 0), (2, 1, 1), shift, full).words.tolist() == [0b10]
    assert _assert_harness(harness, tmp_path, _full_cell_world(shift, True), (0, 0, 0), (2, 1, 1), shift, full).words.tolist() == [0]
    assert _assert_harness(harness, tmp_path, np.ones((64, 64, 64), bool), (65 - 2 * f, 0, 0), (3, 1, 1), shift, f * f).words.tolist() == [0b011]
    # density 1.0: every count at its maximum, the accumulators' slots full
    got = _assert_harness(harness, tmp_path, np.ones((128, 64, 64), bool), (0, 0, 0), (128 >> shift, 2, 2), shift, full)
    assert (got.flat == full).all()
    if shift == 1:
        for nx in (1, 31, 32, 33):
            _assert_harness(harness, tmp_path, _stripe_world(), (0, 0, 0), (nx, 1, 1), 1, 1)


def test_harness_on_every_brick_factor(harness, tmp_path):
    rng = np.random.default_rng(24)
    for factor, shape in [(16, (128, 128, 128)), (32, (256, 256, 256))]:
        world = np.zeros(shape, bool)
        world[:96, :70, :80] = rng.random((96, 70, 80)) < 0.4
        _assert_harness(harness, tmp_path, world, (-5, 3, 7), (13, 9, 10), 3, 5, factor=factor)


def _limits(harness, tmp_path, origin, dims, shift, threshold=1):
    raw, _ = run_harness_files(harness, tmp_path, [1, 8, 64, 64, 64, *origin, *dims, shift, threshold, 0, 0])
    with_o, without, thr, zero = (int(v) for v in np.frombuffer(raw[:16].tobytes(), np.uint32))
    assert zero == 0
    return bool(with_o), bool(without), bool(thr), int(np.frombuffer(raw[16:24].tobytes(), np.uint64)[0])


def test_layout_follows_the_documented_formula_and_limits(harness, tmp_path):
    for shift in SHIFTS:
        for dims in [(1, 1, 1), (3, 1, 1), (31, 5, 7), (33, 3, 3), (100, 7, 9), (1, 1, 1000), (65, 33, 17)]:
            want = R.workspace_bytes(dims, shift)
            assert want > 0 and _limits(harness, tmp_path, (0, 0, 0), dims, shift) == (True, True, True, want)
    for dims in [(0, 1, 1), (1, -1, 1), (1, 1, 0)]:
        assert _limits(harness, tmp_path, (0, 0, 0), dims, 1)[:2] == (False, False) and R.workspace_bytes(dims, 1) == 0
    for shift in (0, 6):  # the shift's ends
        assert _limits(harness, tmp_path, (0, 0, 0), (4, 4, 4), shift) == (False, False, False, 0) and R.workspace_bytes((4, 4, 4), shift) == 0


def test_threshold_limits(harness, tmp_path):
    for shift in SHIFTS:
        full = 1 << (3 * shift)
        assert [_limits(harness, tmp_path, (0, 0, 0), (2, 2, 2), shift, t)[2] for t in (0, 1, full, full + 1)] == [False, True, True, False]
    assert not _limits(harness, tmp_path, (0, 0, 0), (2, 2, 2), 1, -1)[2]


def test_source_limit_of_two_to_the_32(harness, tmp_path):
    """a source product of 2^32 is accepted and the next size refused, at every shift and on every axis"""
    for shift in SHIFTS:
        f = 1 << shift
        edge = [(1 << 32) // (f * f * f * 64 * 64), 64, 64]  # cells: f^3 * product = 2^32
        for k in range(3):
            dims = edge[k:] + edge[:k]
            assert _limits(harness, tmp_path, (0, 0, 0), dims, shift) == (True, True, True, 1 << 29) == (True, True, True, R.workspace_bytes(dims, shift))
            more = list(dims)
            more[(k + 1) % 3] += 1
            assert _limits(harness, tmp_path, (0, 0, 0), more, shift)[:2] == (False, False) and R.workspace_bytes(more, shift) == 0
    # one long axis: S = (2^30, 2, 2) is the limit, and dims near 2^31 do not wrap
    assert _limits(harness, tmp_path, (0, 0, 0), (1 << 29, 1, 1), 1)[:2] == (True, True)
    assert _limits(harness, tmp_path, (0, 0, 0), ((1 << 29) + 1, 1, 1), 1)[:2] == (False, False)
    assert _limits(harness, tmp_path, (0, 0, 0), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), 5)[:2] == (False, False)


def test_layout_accepts_the_last_origin_within_int32(harness, tmp_path):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    dims, shift = (8, 3, 70), 2
    for k in range(3):
        for edge, ok in [(lo, True), (hi - 4 * dims[k], True), (hi - 4 * dims[k] + 1, False), (hi, False)]:
            origin = [0, 0, 0]
            origin[k] = edge
            assert _limits(harness, tmp_path, origin, dims, shift)[:2] == (ok, True)
