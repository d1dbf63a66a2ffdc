"""CPU checks of the stamp orientations (include/vxrt.h, vxrt_orientation_* / vxrt_transform_stamp): the two restatements of
tests/ref_transform.py against each other and on the hand-derived cases of tests/transform_cases.py, the orientation algebra
through the library's C helpers (loaded without a GPU), and the kernels' code (csrc/vxrt_transform.hpp) compiled for the host
(tests/tools/transform_check.cpp) against the restatements -- bits and summary bit-equal, every index checked, every
destination word stored once -- with the limits and the order of the refusals (tests/tools/transform_args_check.cpp)."""
import ctypes as C

import numpy as np
import pytest

from tests import ref_transform as R
from tests import transform_cases as TC
from tests import transform_limit_cases as TL
from tests.helpers import build_harness, run_harness, run_harness_files

ALL = R.all_orientations()
# sd[0] and the source axis that becomes destination x each take every value of {1, 31, 32, 33, 63, 64, 65, 97}
EDGE_SHAPES = [(33, 5, 65), (64, 1, 31), (1, 97, 2), (65, 32, 33), (31, 64, 1), (32, 33, 63), (63, 2, 97), (97, 31, 3), (2, 63, 64),
               (3, 65, 32)]


# ---- the restatements ---------------------------------------------------------------------------------------------------------
def test_edge_shapes_cover_every_width():
    want = {1, 31, 32, 33, 63, 64, 65, 97}
    assert {d[0] for d in EDGE_SHAPES} >= want
    for s in (1, 2):  # the axis a transposing orientation runs destination x along
        assert {d[s] for d in EDGE_SHAPES} >= want


def test_the_restatements_agree_on_random_grids():
    rng = np.random.default_rng(1)
    for d in [(1, 1, 1), (5, 3, 4), (2, 7, 3), (33, 2, 3), (4, 4, 4)]:
        g = rng.random(d) < 0.4
        for o in ALL:
            a, b = R.transform(g, o), R.transform_loop(g, o)
            assert a.shape == R.dims(o, d) and np.array_equal(a, b), (d, o)
            assert int(a.sum()) == int(g.sum())


def test_hand_derived_cases_on_the_restatements():
    for case in TC.written_out():
        g = TC.source_grid(case)
        for f in (R.transform, R.transform_loop):
            out = f(g, case["o"])
            TC.check(case, out.shape, R.pack(out))
    for turn, o in TC.TURNS.items():
        assert R.rotation(*turn) == o and R.is_rotation(o)


def _crops(grid, orientations):
    return [R.crop(R.transform(grid, o)) for o in orientations]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def test_the_tromino_and_the_chiral_piece_under_the_24_rotations():
    """The L-tromino is flat and has a mirror plane: its 24 rotations are 12 shapes and its mirror image is one of them.  The
    piece without symmetry has 24 different rotations, none equal to its mirror image."""
    rot = [o for o in ALL if R.is_rotation(o)]
    assert len(ALL) == 48 and len(rot) == 24
    t = _crops(TC.TROMINO, rot)
    distinct = [a for i, a in enumerate(t) if not any(_same(a, b) for b in t[:i])]
    assert len(distinct) == TC.TROMINO_DISTINCT
    assert any(_same(R.crop(R.transform(TC.TROMINO, ((0, 1, 2), 1))), a) for a in t)
    c = _crops(TC.CHIRAL, rot)
    for i in range(24):
        for j in range(i):
            assert not _same(c[i], c[j]), (rot[i], rot[j])
    for flip in (1, 2, 4, 7):
        m = R.crop(R.transform(TC.CHIRAL, ((0, 1, 2), flip)))
        assert not any(_same(m, a) for a in c)
    assert np.array_equal(R.pack(TC.CHIRAL), np.asarray(TC.CHIRAL_WORDS, np.uint32))
    assert np.array_equal(R.pack(TC.TROMINO), np.asarray(TC.TROMINO_WORDS, np.uint32))


# ---- the algebra through the C helpers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vx():
    import voxelengine_amd as vx
    vx.load()
    return vx


def _o(vx, o):
    return vx.Orientation(tuple(o[0]), o[1])


def _pair(o):
    return tuple(o.axis), o.flip


def test_symbols_and_structs(vx):
    lib = vx.load()
    for name in ("vxrt_orientation_rotation", "vxrt_orientation_compose", "vxrt_orientation_inverse", "vxrt_orientation_dims",
                 "vxrt_orientation_voxel", "vxrt_orientation_is_rotation", "vxrt_transform_stamp", "vxrt_transform_stamp_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    from voxelengine_amd import _native as N
    assert C.sizeof(N.OrientationDesc) == 16 and C.sizeof(N.TransformSummaryDesc) == 32
    assert N.TransformSummaryDesc.set_min.offset == 8 and N.TransformSummaryDesc.set_max.offset == 20
    assert vx.TRANSFORM_MAX_WORDS == 1 << 31 and lib.vxrt_abi_version() == 3


def test_there_are_48_orientations_and_24_rotations(vx):
    every = list(vx.Orientation.all())
    assert sorted(_pair(o) for o in every) == sorted(ALL) and len(set(every)) == 48
    rot = list(vx.Orientation.rotations())
    assert len(rot) == 24 and sorted(_pair(o) for o in rot) == sorted(o for o in ALL if R.is_rotation(o))
    for o in ALL:
        assert _o(vx, o).is_rotation == R.is_rotation(o)


def test_compose_is_transforming_twice(vx):
    g = np.random.default_rng(2).random((3, 4, 5)) < 0.5
    once = {o: R.transform(g, o) for o in ALL}
    for a in ALL:
        for b in ALL:
            ab = _pair(_o(vx, a).then(_o(vx, b)))
            assert ab == R.compose(a, b)
            assert np.array_equal(once[ab], R.transform(once[a], b)), (a, b)


def test_inverse_undoes_every_orientation(vx):
    g = np.random.default_rng(3).random((4, 2, 3)) < 0.5
    for o in ALL:
        inv = _o(vx, o).inverse()
        assert _pair(_o(vx, o).then(inv)) == R.IDENTITY and _pair(inv.then(_o(vx, o))) == R.IDENTITY
        assert np.array_equal(R.transform(R.transform(g, o), _pair(inv)), g)
        assert inv.is_rotation == _o(vx, o).is_rotation


def test_quarter_turns(vx):
    O = vx.Orientation
    assert _pair(O.rotation(2, 1)) == ((1, 0, 2), 1)
    for axis in range(3):
        one = O.rotation(axis, 1)
        assert _pair(one.then(one).then(one).then(one)) == R.IDENTITY and _pair(O.rotation(axis, 0)) == R.IDENTITY
        for n in (-9, -5, -4, -1, 1, 2, 3, 4, 7, 1001, -1001, 2 ** 31 - 1, -2 ** 31, 10 ** 12):
            assert _pair(O.rotation(axis, n)) == R.rotation(axis, n), (axis, n)
            assert O.rotation(axis, n).is_rotation
        for n in (1, 2, 3):
            assert _pair(O.rotation(axis, n)) == TC.TURNS[(axis, n)]
            assert _pair(O.rotation(axis, -n)) == _pair(O.rotation(axis, n).inverse())
    # the 24 rotations are the products of quarter turns
    seen, todo = {R.IDENTITY}, [O()]
    while todo:
        o = todo.pop()
        for axis in range(3):
            n = o.then(O.rotation(axis, 1))
            if _pair(n) not in seen:
                seen.add(_pair(n))
                todo.append(n)
    assert seen == {o for o in ALL if R.is_rotation(o)}
    assert not O.mirror(0).is_rotation and _pair(O.mirror(2)) == ((0, 1, 2), 4)


def test_voxel_and_dims_match_the_rule(vx):
    sd = (3, 4, 5)
    for o in ALL:
        assert _o(vx, o).dims(sd) == R.dims(o, sd)
        for p in [(0, 0, 0), (2, 3, 4), (1, 0, 4), (2, 1, 3)]:
            assert _o(vx, o).voxel(p, sd) == R.voxel(o, sd, p)
    g = np.zeros(sd, bool)
    g[1, 0, 4] = True
    for o in ALL:
        assert R.transform(g, o)[_o(vx, o).voxel((1, 0, 4), sd)]


def test_helpers_refuse_invalid_orientations_and_null(vx):
    from voxelengine_amd import _native as N
    lib = vx.load()
    good = _o(vx, ALL[17])._c()
    out, i3, o3 = N.OrientationDesc(), (C.c_int32 * 3)(3, 4, 5), (C.c_int32 * 3)()
    bad = []
    for axis in [(0, 0, 1), (0, 1, 1), (2, 2, 2), (0, 1, 3), (-1, 1, 2), (0, 1, -2 ** 31), (3, 4, 5), (1, 2, 2 ** 31 - 1)]:
        bad.append(vx.Orientation(axis, 0)._c())
    for flip in (8, 9, 16, 1 << 31, 0xFFFFFFFF):
        bad.append(vx.Orientation((0, 1, 2), flip)._c())
    for b in bad:
        assert lib.vxrt_orientation_compose(C.byref(b), C.byref(good), C.byref(out)) == -1
        assert lib.vxrt_orientation_compose(C.byref(good), C.byref(b), C.byref(out)) == -1
        assert lib.vxrt_orientation_inverse(C.byref(b), C.byref(out)) == -1
        assert lib.vxrt_orientation_dims(C.byref(b), i3, o3) == -1
        assert lib.vxrt_orientation_voxel(C.byref(b), i3, i3, o3) == -1
        assert lib.vxrt_orientation_is_rotation(C.byref(b)) == -1
    assert lib.vxrt_orientation_compose(None, C.byref(good), C.byref(out)) == -1
    assert lib.vxrt_orientation_compose(C.byref(good), None, C.byref(out)) == -1
    assert lib.vxrt_orientation_compose(C.byref(good), C.byref(good), None) == -1
    assert lib.vxrt_orientation_inverse(None, C.byref(out)) == -1 and lib.vxrt_orientation_inverse(C.byref(good), None) == -1
    assert lib.vxrt_orientation_dims(None, i3, o3) == -1 and lib.vxrt_orientation_dims(C.byref(good), None, o3) == -1
    assert lib.vxrt_orientation_dims(C.byref(good), i3, None) == -1
    assert lib.vxrt_orientation_voxel(None, i3, i3, o3) == -1 and lib.vxrt_orientation_voxel(C.byref(good), None, i3, o3) == -1
    assert lib.vxrt_orientation_voxel(C.byref(good), i3, None, o3) == -1 and lib.vxrt_orientation_voxel(C.byref(good), i3, i3, None) == -1
    assert lib.vxrt_orientation_is_rotation(None) == -1
    assert lib.vxrt_orientation_rotation(0, 1, None) == -1
    for axis in (-1, 3, 2 ** 31 - 1, -2 ** 31):
        assert lib.vxrt_orientation_rotation(axis, 1, C.byref(out)) == -1
    assert lib.vxrt_orientation_compose(C.byref(good), C.byref(good), C.byref(good)) == 0  # (out may be an input)
    with pytest.raises(ValueError):
        vx.Orientation((0, 0, 1), 0).inverse()
    with pytest.raises(ValueError):
        vx.Orientation.rotation(3, 1)
    # the device call checks its context first
    assert lib.vxrt_transform_stamp(None, None, None, None, None, None, None) == -1
    assert lib.vxrt_transform_stamp_host(None, None, None, None, None, None) == -1


# ---- the kernels' code on the host -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "transform_check")


def _run(harness, tmp_path, words, sd, o, summary=True, groups=0):
    raw, _ = run_harness_files(harness, tmp_path, [*sd, *o[0], o[1], int(summary), groups], np.asarray(words, np.uint32))
    s = raw[:32].copy()
    box = [int(v) for v in s[8:].view(np.int32)]
    got = (int(s[:8].view(np.uint64)[0]), tuple(box[:3]), tuple(box[3:]))
    return raw[32:].view(np.uint32), got


def _assert_harness(harness, tmp_path, grid, o, summary=True, groups=0):
    want = R.transform(grid, o)
    words, got = _run(harness, tmp_path, R.pack_padded(grid), grid.shape, o, summary, groups)
    assert words.size == len(R.pack(want))
    bits, pad = R.unpack(words, want.shape)
    assert np.array_equal(bits, want), (grid.shape, o)
    assert not pad.any(), (grid.shape, o)
    assert got == (R.summary(want) if summary else (0, (0, 0, 0), (0, 0, 0))), (grid.shape, o)
    return words


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    for case in TC.written_out():
        words, got = _run(harness, tmp_path, case["words"], case["dims"], case["o"])
        TC.check(case, case["want_dims"], words)
        assert got == R.summary(R.unpack(words, case["want_dims"])[0])


@pytest.mark.parametrize("sd", EDGE_SHAPES)
def test_host_code_bit_equal_for_all_48_orientations(harness, tmp_path, sd):
    """padding bits of the source set; bits and summary equal to the restatement; the launch as planned"""
    rng = np.random.default_rng(sum(sd))
    g = rng.random(sd) < 0.3
    for i, o in enumerate(ALL):
        _assert_harness(harness, tmp_path, g, o, summary=i % 5 != 4)


def test_host_code_with_few_workgroups_and_sparse_grids(harness, tmp_path):
    """the stride loops (one and three workgroups), a grid of several tiles on every tile axis, an empty and a full grid, one voxel"""
    rng = np.random.default_rng(9)
    big = rng.random((520, 3, 270)) < 0.2  # 17 x-words: two tiles along x; 270 rows: two tiles of 256 rows
    for o in [((2, 1, 0), 0), ((2, 0, 1), 0b011), ((1, 2, 0), 0b101), ((0, 2, 1), 0b001)]:
        for groups in (0, 1, 3):
            _assert_harness(harness, tmp_path, big if o[0][0] == 2 else big.transpose(0, 2, 1), o, True, groups)
    for o in ALL[::5]:
        for g in (np.zeros((33, 3, 34), bool), np.ones((33, 3, 34), bool)):
            _assert_harness(harness, tmp_path, g, o)
        one = np.zeros((34, 33, 2), bool)
        one[33, 32, 1] = True
        _assert_harness(harness, tmp_path, one, o, True, 2)


def test_argument_limits_without_a_device(tmp_path_factory):
    run_harness(build_harness(tmp_path_factory, "transform_args_check"))


def test_the_limit_case_passes_2_32_bytes_with_few_voxels(vx):
    """tests/transform_limit_cases.py: the shape the GPU suite addresses beyond 32-bit byte offsets"""
    sd = TL.LIMIT_DIMS
    words = vx.region_words(sd)
    assert 4 * words > 1 << 32 and words <= vx.TRANSFORM_MAX_WORDS and sd[0] * sd[1] * sd[2] < (1 << 30) + (1 << 16)
    for o in TL.LIMIT_ORIENTATIONS:
        assert 0 < vx.region_words(R.dims(o, sd)) <= vx.TRANSFORM_MAX_WORDS
    assert vx.region_words(TL.OVER_CAP_DIMS) > vx.TRANSFORM_MAX_WORDS
    assert TL.OVER_CAP_DIMS[0] * TL.OVER_CAP_DIMS[1] * TL.OVER_CAP_DIMS[2] < 1 << 32
    assert {o[0][0] for o in TL.LIMIT_ORIENTATIONS} == {0, 1, 2}  # both kernels, both transposed axes
    import torch
    w = TL.pattern_words(torch, 5000, "cpu").numpy().view(np.uint32)
    assert all(int(w[i]) == (0xFFFFFFFE | TL.pattern_bit(i)) for i in range(5000)) and 1000 < int((w & 1).sum()) < 4000
