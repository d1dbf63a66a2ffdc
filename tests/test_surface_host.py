"""CPU checks of surface extraction (include/vxrt.h, vxrt_extract_surface): the two restatements of tests/ref_surface.py
against each other, the invariants of the definition, the round trip through the voxelization restatements, hand-derived
cases with their packed words written out, and the kernels' per-lane code (csrc/vxrt_surface.hpp) compiled for the host
(tests/tools/surface_check.cpp) against the restatements -- quads, triangles and summary bit-equal, every index checked, the
capacity respected, the workspace formula and the limits of the dims and the origin."""
import numpy as np
import pytest

from tests import ref_surface as R
from tests import ref_voxelize as V
from tests.helpers import build_harness, run_harness_files

# random cases: (world shape, density, origin, dims): boxes inside, partly outside and wholly outside the world
CASES = [((64, 64, 64), 0.01, (0, 0, 0), (16, 8, 16)), ((64, 64, 64), 0.2, (3, 1, 2), (9, 6, 11)), ((64, 64, 64), 0.5, (-3, -2, -1), (12, 7, 9)),
         ((64, 64, 64), 0.8, (57, 59, 58), (12, 9, 10)), ((64, 64, 64), 1.0, (50, 52, 54), (20, 12, 14)), ((64, 64, 64), 0.5, (70, 0, 0), (4, 4, 4)),
         ((64, 64, 64), 0.6, (-9, -9, -9), (5, 5, 5)), ((64, 64, 64), 0.7, (2, 1, 1), (35, 5, 6)), ((128, 64, 64), 0.9, (1, 0, 2), (70, 3, 5)),
         ((64, 64, 64), 0.5, (63, 63, 63), (1, 1, 1)), ((64, 64, 64), 1.0, (-1, -1, -1), (3, 66, 3))]


def _same(a, b):
    assert a.quads.dtype == b.quads.dtype == np.uint32 and a.vertices.dtype == b.vertices.dtype == np.int32
    assert np.array_equal(a.quads, b.quads) and np.array_equal(a.vertices, b.vertices) and np.array_equal(a.triangles, b.triangles)
    assert np.array_equal(a.summary, b.summary), (a.summary, b.summary)


def _both(world, origin, dims, mode):
    a = R.extract(world, origin, dims, mode)
    _same(a, R.extract_scan(world, origin, dims, mode))
    return a


def _worlds():
    rng = np.random.default_rng(11)
    return [(rng.random(shape) < density, origin, dims) for shape, density, origin, dims in CASES]


@pytest.mark.parametrize("mode", [R.CAP, R.OPEN])
def test_the_restatements_agree_on_random_grids(mode):
    for world, origin, dims in _worlds():
        _both(world, origin, dims, mode)


def _check_invariants(world, origin, dims, mode, s):
    d, x, y, z, w, h = R.decode(s.quads)
    fs = R.faces(R.halo_box(world, origin, dims), mode)
    key = np.stack([d, d * 0, d * 0, d * 0], 1)  # canonical order: ascending (d, s, v, u)
    for a in range(3):
        k = (d >> 1) == a
        sv, vv, uv = ((x, z, y), (y, z, x), (z, y, x))[a]
        key[k, 1], key[k, 2], key[k, 3] = sv[k], vv[k], uv[k]
    assert all(tuple(key[i]) < tuple(key[i + 1]) for i in range(len(key) - 1))
    for dd in range(6):
        k = d == dd
        assert int((w[k] * h[k]).sum()) == int(s.summary[4 + dd]) == int(fs[dd].sum())
        assert int(k.sum()) == int(s.summary[10 + dd])
        # the quads of a direction are disjoint and cover its faces
        paint = np.zeros(dims, np.int32)
        for i in np.nonzero(k)[0]:
            ext = [1, 1, 1]
            ext[R._SVU[dd >> 1][2]], ext[R._SVU[dd >> 1][1]] = int(w[i]), int(h[i])
            paint[x[i]:x[i] + ext[0], y[i]:y[i] + ext[1], z[i]:z[i] + ext[2]] += 1
        assert np.array_equal(paint, fs[dd].astype(np.int32))
    if mode == R.CAP:
        assert all(s.summary[4 + 2 * k] == s.summary[5 + 2 * k] for k in range(3))
    # every triangle's normal is a positive multiple of its direction
    p = s.vertices.astype(np.int64)[s.triangles.astype(np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    want = np.asarray(R._STEP, np.int64)[np.repeat(d, 2)]
    area = 65536 * np.repeat(w * h, 2)
    assert np.array_equal(n, want * area[:, None])
    assert np.array_equal(s.triangles[:, 0] // 4, np.repeat(np.arange(len(d)), 2))


@pytest.mark.parametrize("mode", [R.CAP, R.OPEN])
def test_invariants_of_the_definition(mode):
    for world, origin, dims in _worlds():
        _check_invariants(world, origin, dims, mode, R.extract(world, origin, dims, mode))


def _grid(world, origin, dims):
    return R.halo_box(world, origin, dims)[1:-1, 1:-1, 1:-1]


def test_the_cap_surface_voxelizes_back_to_the_box():
    rng = np.random.default_rng(5)
    for density, dims in [(0.2, (7, 5, 6)), (0.5, (34, 4, 5)), (0.8, (9, 8, 7)), (1.0, (5, 6, 33))]:
        world = rng.random((64, 64, 64)) < density
        origin = (2, -1, 3)
        s = R.extract(world, origin, dims, R.CAP)
        want = _grid(world, origin, dims)
        assert np.array_equal(V.voxelize(s.vertices, s.triangles, dims, V.SOLID)["grid"], want)
        if dims[0] * dims[1] * dims[2] < 400:
            assert np.array_equal(V.voxelize_slow(s.vertices, s.triangles, dims, V.SOLID)["grid"], want)


# ---- hand-derived cases: (world, origin, dims, mode, direction filter or None, packed quads) ------------------------------------
def _hand_cases():
    out = {}
    w = np.zeros((64, 64, 64), bool)
    w[1, 2, 3] = True  # pos = 1 | 2 << 10 | 3 << 20, six 1 x 1 quads in direction order
    out["single_voxel"] = (w, (0, 0, 0), (4, 4, 4), R.CAP, None, [(0x300801, d << 20) for d in range(6)])
    w = np.zeros((64, 64, 64), bool)
    w[1:6, 1:4, 1:5] = True  # a 5 x 3 x 4 box: -x, +x are 3 x 4 (y, z), -y, +y are 5 x 4 (x, z), -z, +z are 5 x 3 (x, y)
    out["solid_box"] = (w, (0, 0, 0), (7, 5, 6), R.CAP, None,
                        [(0x100401, 0x000C02), (0x100405, 0x100C02), (0x100401, 0x200C04), (0x100C01, 0x300C04),
                         (0x100401, 0x400804), (0x400401, 0x500804)])
    w = np.zeros((64, 64, 64), bool)
    w[2:5, 0, 0], w[2:6, 1, 0], w[2:5, 2, 0] = True, True, True  # +z: rows y = 0, 1, 2 hold [2, 5), [2, 6), [2, 5)
    out["three_rows"] = (w, (0, 0, 0), (8, 8, 8), R.CAP, 5, [(0x002, 0x500002), (0x402, 0x500003), (0x802, 0x500002)])
    w = np.zeros((64, 64, 64), bool)
    w[1:5, 0, 0], w[2:5, 1, 0] = True, True  # [1, 5) above [2, 5): not merged
    out["shifted_start"] = (w, (0, 0, 0), (8, 8, 8), R.CAP, 5, [(0x001, 0x500003), (0x402, 0x500002)])
    w = np.zeros((64, 64, 64), bool)
    w[2:5, 0:2, 0] = True  # two stacked identical runs: one quad, h = 2
    out["stacked"] = (w, (0, 0, 0), (8, 8, 8), R.CAP, 5, [(0x002, 0x500402)])
    return out


@pytest.mark.parametrize("name", ["single_voxel", "solid_box", "three_rows", "shifted_start", "stacked"])
def test_hand_derived_quads(name):
    world, origin, dims, mode, only, want = _hand_cases()[name]
    q = _both(world, origin, dims, mode).quads
    if only is not None:
        q = q[q[:, 1] >> 20 == only]
    assert [(int(a), int(b)) for a, b in q] == want


def _checkerboard():
    g = np.indices((64, 64, 64)).sum(0) % 2 == 0
    return g, (1, 0, 2), (6, 7, 5)


def _floor_slab():
    w = np.zeros((64, 64, 64), bool)
    w[:, :2, :] = True
    return w, (4, 0, 4), (4, 4, 4)


def _half_outside():
    w = np.zeros((64, 64, 64), bool)
    w[56:, :8, :8] = True
    return w, (60, 0, 0), (8, 8, 8)


def _check_checkerboard(cap):
    solid = int(cap.summary[0])
    assert solid == int(_grid(*_checkerboard()).sum()) and cap.summary[1] == cap.summary[2] == 6 * solid
    assert (cap.quads[:, 1] & 0xFFFFF == 0).all()


def _check_floor_slab(cap, opn):
    # CAP: a wall of 2 x 4 faces on each side, one quad each; the floor's underside lies on the world's edge in both modes
    assert list(cap.summary[4:10]) == [8, 8, 16, 16, 8, 8] and list(cap.summary[10:16]) == [1] * 6
    assert list(opn.summary[4:10]) == [0, 0, 16, 16, 0, 0] and list(opn.summary[10:16]) == [0, 0, 1, 1, 0, 0]
    assert [(int(a), int(b)) for a, b in opn.quads] == [(0x0, 0x200C03), (0x400, 0x300C03)]


def _check_half_outside(cap, opn):
    # the world ends at box x = 4: a wall there in both modes, and on the world's y and z edges; CAP adds the wall at x = 0
    assert list(opn.summary[4:10]) == [0, 64, 32, 32, 32, 32] and list(cap.summary[4:10]) == [64, 64, 32, 32, 32, 32]
    assert (0x3, 0x101C07) in [(int(a), int(b)) for a, b in opn.quads] and opn.summary[0] == 256


def test_hand_derived_worlds():
    _check_checkerboard(_both(*_checkerboard(), R.CAP))
    _check_floor_slab(_both(*_floor_slab(), R.CAP), _both(*_floor_slab(), R.OPEN))
    _check_half_outside(_both(*_half_outside(), R.CAP), _both(*_half_outside(), R.OPEN))


# ---- the kernels' code on the host ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "surface_check")


def _run_harness(harness, tmp_path, world, factor, origin, dims, mode, capacity, triangles=True):
    from oracle import vxo
    X, Y, Z = world.shape
    header = [0, factor, X, Y, Z, *origin, *dims, mode, capacity, int(triangles)]
    raw, _ = run_harness_files(harness, tmp_path, header, vxo.dense_from_voxels(world))
    words = np.frombuffer(raw.tobytes(), np.uint32)
    summary = words[:16].copy()
    n = int(summary[3])
    quads = words[16:16 + 2 * n].reshape(-1, 2)
    if not triangles:
        assert len(words) == 16 + 2 * n
        return R.Surface(quads, np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), summary)
    assert len(words) == 16 + 20 * n
    return R.Surface(quads, words[16 + 2 * n:16 + 14 * n].view(np.int32).reshape(-1, 3), words[16 + 14 * n:].reshape(-1, 3), summary)


def _assert_harness(harness, tmp_path, world, origin, dims, mode, factor=8):
    want = R.extract(world, origin, dims, mode)
    _same(_run_harness(harness, tmp_path, world, factor, origin, dims, mode, len(want.quads) + 3), want)
    return want


@pytest.mark.parametrize("mode", [R.CAP, R.OPEN])
def test_harness_equals_the_restatements_on_random_grids(harness, tmp_path, mode):
    for world, origin, dims in _worlds():
        _assert_harness(harness, tmp_path, world, origin, dims, mode)


@pytest.mark.parametrize("mode", [R.CAP, R.OPEN])
def test_harness_runs_across_words_and_waves(harness, tmp_path, mode):
    """box widths around one and two halo words and around the 64 lanes of a wave; runs that cross x = 30 .. 34"""
    rng = np.random.default_rng(21)
    world = rng.random((128, 64, 64)) < 0.85
    world[28:36] |= rng.random((8, 64, 64)) < 0.7
    for ox, dx in [(0, 1), (3, 30), (1, 31), (0, 32), (-1, 33), (2, 62), (5, 63), (0, 64), (-2, 65), (7, 80)]:
        _assert_harness(harness, tmp_path, world, (ox, -1, 1), (dx, 6, 7), mode)


def test_harness_on_the_hand_derived_worlds(harness, tmp_path):
    for name, (world, origin, dims, mode, only, want) in _hand_cases().items():
        q = _assert_harness(harness, tmp_path, world, origin, dims, mode).quads
        assert [(int(a), int(b)) for a, b in (q if only is None else q[q[:, 1] >> 20 == only])] == want
    _check_checkerboard(_assert_harness(harness, tmp_path, *_checkerboard(), R.CAP))
    _check_floor_slab(_assert_harness(harness, tmp_path, *_floor_slab(), R.CAP), _assert_harness(harness, tmp_path, *_floor_slab(), R.OPEN))
    _check_half_outside(_assert_harness(harness, tmp_path, *_half_outside(), R.CAP),
                        _assert_harness(harness, tmp_path, *_half_outside(), R.OPEN))


def test_harness_respects_the_capacity(harness, tmp_path):
    """0, 1, quads - 1, quads, quads + 7: the harness itself checks that nothing past `written` records is touched"""
    world, origin, dims = _worlds()[2]
    want = R.extract(world, origin, dims, R.CAP)
    n = len(want.quads)
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 7):
        for tri in (True, False):
            got = _run_harness(harness, tmp_path, world, 8, origin, dims, R.CAP, cap, tri)
            cut = want.cut(cap)
            assert np.array_equal(got.summary, cut.summary) and np.array_equal(got.quads, cut.quads)
            if tri:
                _same(got, cut)


def test_harness_at_the_field_limits(harness, tmp_path):
    """a solid bar of 1024 voxels on each axis: w - 1 = 1023 along x and y, h - 1 = 1023 along y and z"""
    for k in range(3):
        shape, dims = [64, 64, 64], [1, 1, 1]
        shape[k] = dims[k] = 1024
        want = _assert_harness(harness, tmp_path, np.ones(shape, bool), (0, 0, 0), tuple(dims), R.CAP)
        assert len(want.quads) == 6 and int(want.summary[1]) == 4 * 1024 + 2
        assert {int(e) & 0xFFFFF for e in want.quads[:, 1]} == [{0, 1023}, {0, 1023, 1023 << 10}, {0, 1023 << 10}][k]


def _layout(harness, tmp_path, origin, dims):
    raw, _ = run_harness_files(harness, tmp_path, [1, 8, 64, 64, 64, *origin, *dims, 0, 0, 0])
    with_o, without = (int(v) for v in np.frombuffer(raw[:8].tobytes(), np.uint32))
    return bool(with_o), bool(without), int(np.frombuffer(raw[8:16].tobytes(), np.uint64)[0])


def workspace_bytes(dims):
    """the formula of include/vxrt.h"""
    r = lambda n: -(-n // 256) * 256
    if any(d < 1 or d > 1024 for d in dims) or dims[0] * dims[1] * dims[2] > 1 << 28:
        return 0
    H = -(-(dims[0] + 2) // 32) * (dims[1] + 2) * (dims[2] + 2)
    rows = 2 * dims[2] * (dims[0] + 2 * dims[1])
    return r(4 * H) + r(4 * rows) + r(4 * -(-rows // 256))


def test_layout_follows_the_documented_formula_and_limits(harness, tmp_path):
    for dims in [(1, 1, 1), (30, 1, 1), (31, 5, 7), (62, 3, 3), (63, 3, 3), (1024, 1, 1), (1, 1024, 1), (1, 1, 1024), (1024, 1024, 256),
                 (640, 640, 640), (96, 160, 112)]:
        assert _layout(harness, tmp_path, (0, 0, 0), dims) == (True, True, workspace_bytes(dims)) and workspace_bytes(dims) > 0
    for dims in [(0, 1, 1), (1, -1, 1), (1, 1, 0), (1025, 1, 1), (1, 1025, 1), (1, 1, 1025), (1024, 1024, 257), (656, 640, 640)]:
        assert _layout(harness, tmp_path, (0, 0, 0), dims) == (False, False, 0) and workspace_bytes(dims) == 0


def test_layout_accepts_the_last_origin_whose_halo_fits_int32(harness, tmp_path):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    for dims in [(8, 3, 70), (1, 1, 1), (33, 2, 2)]:
        for k in range(3):
            for edge, ok in [(lo + 1, True), (lo, False), (hi - dims[k] - 1, True), (hi - dims[k], False)]:
                origin = [0, 0, 0]
                origin[k] = edge
                assert _layout(harness, tmp_path, origin, dims)[:2] == (ok, True), (dims, k, edge)
