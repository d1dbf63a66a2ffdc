"""The launch-limit cases of voxelization and distance fields (tests/launch_limit_cases.py) without a GPU: the constants
read from the sources, every case past what it targets (and a copy of the sources with any one constant raised leaving some
case short), the radius cases on both sides of each threshold of distance_field, and what the GPU test takes for granted held
against the restatements: the identities that stand in for a full voxelization (copies of a mesh, inert triangles, 2^20
degenerate triangles), the k = 53 cases through the kernels' code on the host (tests/tools/voxelize_check.cpp), the runs of
the row-width meshes, distance_field_points against the halo forms and brute force, and per radius case the conditions that
make the outermost rows of a slab decide a value."""
import os
import re

import numpy as np
import pytest

from tests import launch_limit_cases as L
from tests import ref_dist as RD
from tests import ref_voxelize as RV
from tests.test_voxelize_host import _assert_harness, harness  # noqa: F401  (the fixture that builds voxelize_check)


def _short(caps):
    return [(case.name, what, value, bound) for case in L.LAUNCH_CASES for what, value, bound in case.reach(caps)
            if not value > bound]


# ---- the constants ---------------------------------------------------------------------------------------------------------
def test_constants_are_read_from_the_sources():
    c = L.read_caps()
    assert all(v > 0 for v in c.values())
    assert c["dist_small_radius"] < c["dist_mid_radius"] < c["dist_max_radius"] == RD.MAX_RADIUS
    assert (c["vox_max_dim"], c["vox_max_coord"]) == (RV.MAX_DIM, RV.MAX_COORD)


@pytest.mark.parametrize("case", L.LAUNCH_CASES, ids=[c.name for c in L.LAUNCH_CASES])
def test_case_exceeds_what_it_targets(case):
    caps = L.read_caps()
    reach = case.reach(caps)
    assert reach
    for what, value, bound in reach:
        assert value > bound, (case.name, what, value, bound)


def test_radius_cases_stand_on_both_sides_of_each_threshold():
    sides = L.radius_sides(L.read_caps())
    assert len(sides) == 2
    for threshold, (at, past) in sides.items():
        assert len(at) == 1 and len(past) == 1, (threshold, at, past)
    assert L.read_caps()["dist_max_radius"] in L.RADII


@pytest.mark.parametrize("name", sorted(L.CAP_SOURCES))
def test_a_raised_constant_leaves_a_case_short(tmp_path, name):
    """each constant multiplied by 64 (a shift count: 64-fold) in a copy of its source: some case no longer exceeds it"""
    for path, _, _ in L.CAP_SOURCES.values():
        dst = tmp_path / path
        dst.parent.mkdir(parents=True, exist_ok=True)
        with open(os.path.join(L.ROOT, path)) as f:
            dst.write_text(f.read())
    path, rx, _ = L.CAP_SOURCES[name]
    text = (tmp_path / path).read_text()
    m = re.search(rx, text)
    raised = m.group(0).replace(m.group(1), str(int(m.group(1)) * 64))
    (tmp_path / path).write_text(text.replace(m.group(0), raised))
    caps = L.read_caps(str(tmp_path))
    assert caps[name] >= 64 * L.read_caps()[name]
    assert _short(caps), name
    assert not _short(L.read_caps())


# ---- voxelization: copies, inert triangles, the triangle limit -----------------------------------------------------------------
def _equal(got, want):
    return np.array_equal(got["grid"], want["grid"]) and got["summary"] == want["summary"]


@pytest.mark.parametrize("k", [3, 2])
def test_copies_and_inert_blocks_equal_the_reference(k):
    """the tiling identity and the inert-filler identity against the restatement of the whole mesh"""
    mesh = L.copies(k)
    assert len(mesh[1]) == k * 1280
    blocks = [(0, 7), (1000, 800), (len(mesh[1]), 9)]
    more, extra, inert = L.with_inert_blocks(mesh, L.BASE_DIMS, blocks)
    assert extra[0] == 816 == inert.sum() and min(extra[1:]) > 200 and inert[:7].all() and inert[-9:].all() and inert[1007:1807].all()
    for modes in L.MODES:
        want = L.expected_copies(k, modes)
        assert _equal(RV.voxelize(*mesh, L.BASE_DIMS, modes), want), (k, modes)
        assert _equal(RV.voxelize(*more, L.BASE_DIMS, modes), L.expected_copies(k, modes, extra)), (k, modes)
        assert want["summary"][3] == k * 1280 and want["summary"][1] == (L.base_reference(RV.SURFACE)["summary"][1] if modes & 1 else 0)
    assert L.expected_copies(2, RV.SOLID)["summary"][:3] == (0, 0, 0)
    assert L.expected_copies(3, RV.SOLID)["summary"][0] == L.base_reference(RV.SOLID)["summary"][0] > 10000


def test_shuffled_case_leaves_whole_shares_without_an_item():
    caps = L.read_caps()
    mesh, extra, inert = L.shuffled_copies()
    assert len(mesh[1]) == L._SHUFFLED_NT == 53 * 1280 + extra[0] and inert.sum() == extra[0]
    ngroups, per, owners = L.group_shares(len(inert), caps)
    empty = L.empty_shares(inert, caps)
    assert per == 2 and len(empty) >= 4 and 0 in empty and owners - 1 in empty, (ngroups, per, owners, empty)
    assert sorted(np.unique(mesh[1][~inert], axis=0).tolist()) == sorted(L.base_mesh()[1].tolist())  # every base triangle is there
    # runs of empty groups in the middle, for vox_find to step over
    g = np.add.reduceat(~inert, np.arange(0, len(inert), caps["vox_group"]))
    runs = np.flatnonzero((g[1:-1] == 0) & (g[:-2] == 0) & (g[2:] == 0))
    assert len(runs) >= 4


def test_copies_53_through_the_kernels_code_on_the_host(harness, tmp_path):  # noqa: F811
    plain, (shuffled, extra, _) = L.copies(53), L.shuffled_copies()
    for modes in L.MODES:
        _assert_harness(harness, tmp_path, plain, L.BASE_DIMS, modes, L.expected_copies(53, modes))
        _assert_harness(harness, tmp_path, shuffled, L.BASE_DIMS, modes, L.expected_copies(53, modes, extra))


def test_degenerate_triangles_are_inert_at_2_20():
    nt = 1 << 20
    mesh = L.scattered_in_degenerates(nt)
    pos = L.limit_positions(nt)
    assert pos[0] == 0 and pos[-1] == nt - 1 and len(np.unique(pos)) == 1280 and (np.diff(pos) > 256).all()
    assert _equal(RV.voxelize(*mesh, L.BASE_DIMS, 3), L.expected_copies(1, 3, (nt - 1280, 0, nt - 1280, 0)))


# ---- voxelization: row widths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d0", L.ROW_WIDTHS + ("wide",))
def test_row_meshes_toggle_in_many_words_of_a_row(d0):
    mesh, dims = L.row_case(d0)
    wpr = L.ceil_div(dims[0], 32)
    for modes in L.ROW_MODES:
        r = L.row_reference(d0, modes)
        assert 0 < r["summary"][0] and r["summary"][2] < dims[0] * dims[1] * dims[2]
        assert r["summary"][3:6] == (len(mesh[1]), 0, 0)                     # every triangle valid, the coordinate limit kept
        words = RV.pack(r["grid"]).reshape(-1, wpr)
        if dims[0] % 32:
            assert not (words[:, -1] >> np.uint32(dims[0] % 32)).any()       # the padding bits are 0
        assert np.array_equal(RV.unpack(words.reshape(-1), dims), r["grid"])
    solid = L.row_reference(d0, RV.SOLID)["grid"]
    if wpr >= 2:  # the first voxel of a row's last word is the parity of that word's toggles: odd in some rows, even in others
        top = solid[32 * (wpr - 1)]
        assert top.any() and not top.all(), d0
    starts, ends = L.run_words(solid)
    if wpr >= 3:
        assert ((starts >= 3) & (ends >= 3)).any(), (d0, int(starts.max()), int(ends.max()))
    else:
        assert starts.max() >= 1


# ---- distance fields: the reference for large radii ------------------------------------------------------------------------------
def _dense(shape, solid, points):
    w = np.full(shape, bool(solid))
    for p in points:
        w[p] = not solid
    return w


def test_dense_world_words_equal_the_oracles_layout(vxo):
    pts = [(0, 0, 0), (7, 8, 9), (23, 15, 31), (8, 0, 0), (16, 8, 24)]
    for solid in (False, True):
        assert np.array_equal(L.dense_world((24, 16, 32), solid, pts), vxo.dense_from_voxels(_dense((24, 16, 32), solid, pts)))


@pytest.mark.parametrize("mode", L.DIST_MODES)
@pytest.mark.parametrize("radius", [1, 7, 33])
def test_points_form_equals_the_halo_forms_and_brute_force(radius, mode):
    shape = (24, 20, 24)
    rng = np.random.default_rng(radius + 100 * mode)
    pts = [tuple(int(c) for c in p) for p in np.unique(rng.integers(0, shape, (7, 3)), axis=0)]
    world = _dense(shape, mode == RD.TO_EMPTY, pts)
    listed = pts + [(-3, 2, 2), (5, 40, 5)]  # outside the world: no target of TO_SOLID, nothing new for TO_EMPTY
    for origin, dims in [((2, 3, 4), (6, 5, 4)), ((-5, -2, 18), (7, 4, 9)), ((20, 17, -4), (6, 5, 7)), ((9, 9, 9), (1, 3, 2)),
                         ((-40, 5, 5), (5, 3, 2)), ((0, 0, 0), shape)]:
        got = RD.distance_field_points(shape, listed, origin, dims, radius, mode)
        want = RD.distance_field(world, origin, dims, radius, mode)
        assert np.array_equal(got["dist2"], want["dist2"]) and got["summary"] == want["summary"], (origin, dims)
        if dims[0] * dims[1] * dims[2] <= 400:
            brute = RD.distance_field_brute(world, origin, dims, radius, mode)
            assert np.array_equal(got["dist2"], brute["dist2"]) and got["summary"] == brute["summary"], (origin, dims)


# ---- distance fields: the radius cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", L.DIST_MODES)
@pytest.mark.parametrize("group", sorted(L.RADIUS_GROUPS))
def test_radius_cases_let_the_outermost_rows_decide(group, mode):
    caps = L.read_caps()
    shape, origin, targets = L.radius_case(group, mode)
    assert 10 <= len(targets) <= 30 and len(set(targets)) == len(targets), len(targets)
    assert all(d > caps["dist_tile"] and d % caps["dist_tile"] for d in L.RADIUS_BOX)
    fields = {}
    for R in L.RADIUS_GROUPS[group]:
        assert min(o - R for o in origin) < 0                                   # the halo starts outside the world
        r = fields[R] = L.radius_reference(group, R, mode)
        zero, near, far, max_d2, _ = r["summary"]
        assert far > 0 and near > 0 and max_d2 > (R - 1) ** 2, (R, r["summary"])
        for axis in (1, 2):
            assert L.nearest_along_one_axis(group, R, mode, axis), (R, axis)
        if mode == RD.TO_EMPTY:                                                 # the world's outside is within R of part of the box
            assert zero > 0 or (r["dist2"][0] != RD.FAR).all()
    if group == "large":  # a target in the halo past the last tile on +y and +z decides the box's last voxel
        q = int(0.7 * 255)
        corner = tuple(o + d - 1 + k for o, d, k in zip(origin, L.RADIUS_BOX, (0, q, q)))
        assert corner in targets and q > caps["dist_tile"] and fields[255]["dist2"][-1, -1, -1] == 2 * q * q
    else:                 # wherever the smaller radius gives a value, the larger one gives the same
        a, b = (fields[R]["dist2"] for R in L.RADIUS_GROUPS[group])
        assert np.array_equal(a[a != RD.FAR], b[a != RD.FAR]) and (b != RD.FAR).sum() > (a != RD.FAR).sum()
