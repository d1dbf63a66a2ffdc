"""CPU checks of mesh voxelization (include/vxrt.h, vxrt_voxelize_mesh): the restatements of tests/ref_voxelize.py against
each other (the integer separating-axis test against exact rational clipping on every case small enough for it, the per-voxel
sign form against the threshold form on every case here) and on hand-derived cases, and the kernels' code (csrc/vxrt_voxelize.hpp) compiled for the host with
-ftrapv (tests/tools/voxelize_check.cpp) against them -- bits and summary bit-equal, every index checked, the hierarchical
cull on and off, the work items in both orders, the workspace formula, the coordinate limits and the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ref_voxelize as R
from tests.helpers import ROOT, run_harness_files
from tests.launch_limit_cases import coordinate_limit_dims, coordinate_limit_meshes

MODES = (R.SURFACE, R.SOLID, R.SURFACE | R.SOLID)
U = R.UNIT


# ---- the cases: name -> (mesh, dims); the small ones are also run through the slow restatements -----------------------------
def _small_cases():
    return {
        "box_on_centres": (R.box_mesh((U + 128,) * 3, (5 * U + 128, 4 * U + 128, 6 * U + 128)), (8, 7, 9)),
        "box_on_boundaries": (R.box_mesh((2 * U, U, 3 * U), (6 * U, 5 * U, 7 * U)), (9, 8, 8)),
        "box_partly_outside": (R.box_mesh((-500, 300, -77), (1500, 5000, 900)), (7, 6, 5)),
        "box_generic": (R.box_mesh((131, 377, 201), (1711, 1403, 1999)), (8, 8, 9)),
        "octahedron_on_centres": (R.octahedron((5 * U + 128, 4 * U + 128, 4 * U + 128), 3 * U), (11, 9, 10)),
        "octahedron_negative": (R.octahedron((100, 300, -200), 900), (6, 6, 6)),
        "icosphere_80": (R.icosphere((5.3, 4.9, 5.1), 4.2, 1), (11, 10, 11)),
        "torus": (R.torus((7.0, 3.0, 7.0), 4.5, 1.6, 10, 6), (14, 6, 14)),
        "heightfield": (R.heightfield(4, 3, 2.5, 4.0, 3), (10, 5, 8)),
        "soup": (R.soup(60, (9, 7, 8), 2.0, 5), (9, 7, 8)),
        "soup_snapped_thin": (R.soup(40, (33, 3, 4), 3.0, 6), (33, 3, 4)),
    }


def _large_cases():
    big = np.array([[-3000, -2000, 900], [52000, 30000, 12000], [1000, 39000, 26000]], np.int32)
    return {
        "icosphere_1280": (R.icosphere((24.2, 23.7, 24.4), 20.3, 3), (48, 47, 49)),
        "torus_fine": (R.torus((35.0, 9.5, 30.0), 22.0, 7.3, 40, 16), (70, 19, 61)),
        "heightfield_wide": (R.heightfield(12, 9, 6.0, 14.0, 7), (72, 16, 54)),
        "soup_500": (R.soup(500, (70, 33, 40), 3.0, 8), (70, 33, 40)),
        "one_large_triangle": ((big, np.array([[0, 1, 2]], np.uint32)), (200, 150, 100)),
        "soup_long_rows": (R.soup(80, (300, 9, 7), 30.0, 9), (300, 9, 7)),
    }


SMALL, LARGE = _small_cases(), _large_cases()


def _both(mesh, dims, modes):
    """both restatements of each field, asserted equal; returns the fast one"""
    a, b = R.voxelize(*mesh, dims, modes), R.voxelize_slow(*mesh, dims, modes)
    assert np.array_equal(a["grid"], b["grid"]) and a["summary"] == b["summary"]
    return a


_fast_cache = {}


def _fast_and_sign(mesh, dims, modes):
    """the fast pair, its solid field asserted equal to the per-voxel sign form (rational clipping is left to the small cases)"""
    a = R.voxelize(*mesh, dims, modes)
    if modes == R.SOLID:
        assert np.array_equal(a["grid"], R.solid_sign(*mesh, dims))
    return a


def _want(name, modes):
    if (name, modes) not in _fast_cache:
        mesh, dims = {**SMALL, **LARGE}[name]
        _fast_cache[name, modes] = _both(mesh, dims, modes) if name in SMALL else _fast_and_sign(mesh, dims, modes)
    return _fast_cache[name, modes]


# ---- the kernels' code on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("voxelize_check") / "voxelize_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ftrapv", "-I" + os.path.join(ROOT, "tests", "tools", "hoststub"), "-o", exe,
                           os.path.join(ROOT, "tests", "tools", "voxelize_check.cpp"), "-w"])
    return exe


def _run_harness(harness, tmp_path, mesh, dims, modes, cull=1, reverse=0):
    v, t = np.ascontiguousarray(mesh[0], np.int32).reshape(-1, 3), np.ascontiguousarray(mesh[1], np.uint32).reshape(-1, 3)
    raw, _ = run_harness_files(harness, tmp_path, [0, *dims, modes, cull, reverse, len(v), len(t)], v, t)
    s = np.frombuffer(raw[:32].tobytes(), np.uint32)
    q = np.frombuffer(raw[32:32 + 88].tobytes(), np.uint64)
    words = np.frombuffer(raw[120:].tobytes(), np.uint32)
    wpr = (dims[0] + 31) // 32
    assert len(words) == wpr * dims[1] * dims[2]
    grid = R.unpack(words, dims)
    assert np.array_equal(R.pack(grid), words), "padding bits set"
    return {"grid": grid, "summary": tuple(int(x) for x in s[:7]), "items": int(q[0]), "ballots": [int(x) for x in q[1:4]],
            "top": [int(x) for x in q[4:10]], "bytes": int(q[10])}


def _assert_harness(harness, tmp_path, mesh, dims, modes, want, **kw):
    got = _run_harness(harness, tmp_path, mesh, dims, modes, **kw)
    assert np.array_equal(got["grid"], want["grid"]), (dims, modes, kw)
    assert got["summary"] == want["summary"], (dims, modes, kw)
    assert got["bytes"] == R.workspace_bytes(dims, len(mesh[1]))
    return got


# ---- the restatements -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_restatements_agree(harness, tmp_path, name):
    for modes in MODES:
        r = _want(name, modes)
        s = r["summary"]
        assert s[0] == r["grid"].sum() and s[0] <= s[1] + s[2] and s[3] == len(SMALL[name][0][1])
        _assert_harness(harness, tmp_path, *SMALL[name], modes, r)
    assert np.array_equal(_want(name, 3)["grid"], _want(name, 1)["grid"] | _want(name, 2)["grid"])  # SOLID | SURFACE is the OR


def test_sat_equals_rational_clipping_pair_by_pair(harness, tmp_path):
    """triangles with vertices on the half-voxel lattice against the 216 cubes around them: many exact ties; the kernels' test
    on the same triangles"""
    rng = np.random.default_rng(12)
    pairs = ties = 0
    for _ in range(60):
        p = (rng.integers(0, 7, (3, 3)) * 128 + 256).astype(np.int64)
        if not R._normal(p).any():
            continue
        g = np.zeros((6, 6, 6), bool)
        R._surface_tri(g, p)
        for v in np.ndindex(6, 6, 6):
            hit = R.triangle_meets_cube(p, v)
            assert hit == g[v], (p.tolist(), v)
            pairs += 1
            ties += hit
        mesh = (p.astype(np.int32), np.array([[0, 1, 2]], np.uint32))
        assert np.array_equal(_run_harness(harness, tmp_path, mesh, (6, 6, 6), R.SURFACE)["grid"], g), p.tolist()
    assert pairs > 10000 and ties > 500


def _centres_in(a, b, dims):
    m = [(U * np.arange(d) + 128 >= lo) & (U * np.arange(d) + 128 < hi) for d, lo, hi in zip(dims, a, b)]
    return m[0][:, None, None] & m[1][None, :, None] & m[2][None, None, :]


BOXES = [((U + 128,) * 3, (5 * U + 128, 4 * U + 128, 6 * U + 128), (8, 7, 9)),      # faces through voxel centres
         ((2 * U, U, 3 * U), (6 * U, 5 * U, 7 * U), (9, 8, 8)),                      # faces on voxel boundaries
         ((-500, 300, -77), (1500, 5000, 900), (7, 6, 5)),                           # partly outside
         ((-3000, -3000, -3000), (90000, 90000, 90000), (5, 4, 3)),                  # the region inside the box
         ((3000, 100, 100), (4000, 900, 900), (5, 4, 4)),                            # beyond the +x face
         ((-4000, 100, 100), (-3000, 900, 900), (5, 4, 4))]                          # beyond the -x face


def _check_box(grid, a, b, dims):
    assert np.array_equal(grid, _centres_in(a, b, dims)), (a, b)


def _check_plane_triangle(grid):
    want = np.zeros((6, 5, 5), bool)
    for x in (2, 3):
        for y, z in ((1, 1), (2, 1), (1, 2)):
            want[x, y, z] = True
    assert np.array_equal(grid, want)


PLANE_TRIANGLE = (np.array([[768, 300, 300], [768, 700, 300], [768, 300, 700]], np.int32), np.array([[0, 1, 2]], np.uint32))
CORNER_TRIANGLE = (np.array([[768, 768, 768], [1000, 800, 900], [900, 1000, 800]], np.int32), np.array([[0, 1, 2]], np.uint32))


def _check_corner_triangle(grid):
    assert grid[2:4, 2:4, 2:4].all() and not grid[:2].any() and not grid[:, :2].any() and not grid[:, :, :2].any()


def _perturbed_octahedron(c, r, dims):
    """the point (cx + eta, cy + eps, cz + eps^2), 0 < eps << eta << 1, inside |x| + |y| + |z| < r around c: the distance sum
    is S + s(dx) eta + .., s(0) = +1, so a centre with S == r is inside exactly when dx < 0"""
    g = [U * np.arange(d) + 128 - ck for d, ck in zip(dims, c)]
    dx, dy, dz = g[0][:, None, None], g[1][None, :, None], g[2][None, None, :]
    s = np.abs(dx) + np.abs(dy) + np.abs(dz)
    return (s < r) | ((s == r) & (dx < 0))


def test_hand_derived_cases(harness, tmp_path):
    """each case on both restatements and on the kernels' code"""
    def all_three(mesh, dims, modes):
        return _assert_harness(harness, tmp_path, mesh, dims, modes, _both(mesh, dims, modes))["grid"]
    for a, b, dims in BOXES:
        _check_box(all_three(R.box_mesh(a, b), dims, R.SOLID), a, b, dims)
    _check_plane_triangle(all_three(PLANE_TRIANGLE, (6, 5, 5), R.SURFACE))
    _check_corner_triangle(all_three(CORNER_TRIANGLE, (5, 5, 5), R.SURFACE))
    mesh, dims = SMALL["octahedron_on_centres"]
    want = _perturbed_octahedron((5 * U + 128, 4 * U + 128, 4 * U + 128), 3 * U, dims)
    assert np.array_equal(all_three(mesh, dims, R.SOLID), want) and want.sum() > 30
    assert (want ^ _perturbed_octahedron((5 * U + 128, 4 * U + 128, 4 * U + 128), 3 * U + 1, dims)).sum() > 20  # ties occur


def _variants(mesh, seed):
    """the same mesh with its triangles shuffled, its vertex order rotated and its winding flipped"""
    v, t = mesh
    rng = np.random.default_rng(seed)
    yield v, t[rng.permutation(len(t))]
    yield v, np.ascontiguousarray(t[:, [1, 2, 0]])
    yield v, np.ascontiguousarray(t[:, [0, 2, 1]])
    mixed = t.copy()
    flip = rng.random(len(t)) < 0.5
    mixed[flip] = mixed[flip][:, [2, 1, 0]]
    yield v, mixed


@pytest.mark.parametrize("name", ["octahedron_on_centres", "icosphere_80", "soup", "box_on_centres"])
def test_invariance_and_translation(harness, tmp_path, name):
    mesh, dims = SMALL[name]
    for modes in MODES:
        want = _want(name, modes)
        for i, m in enumerate(_variants(mesh, 3)):
            got = R.voxelize(*m, dims, modes)
            assert np.array_equal(got["grid"], want["grid"]) and got["summary"] == want["summary"], (modes, i)
        # the mesh and the region moved by whole voxels: the same voxels, moved
        shift, grow = np.array([2, 1, 3]), (dims[0] + 4, dims[1] + 3, dims[2] + 3)
        moved = R.voxelize(mesh[0] + U * shift, mesh[1], grow, modes)["grid"]
        clipped = R.voxelize(mesh[0], mesh[1], (grow[0] - 2, grow[1] - 1, grow[2] - 3), modes)["grid"]
        assert np.array_equal(moved[2:, 1:, 3:], clipped)
        assert np.array_equal(_run_harness(harness, tmp_path, (mesh[0] + U * shift.astype(np.int32), mesh[1]), grow, modes)["grid"], moved)
        assert np.array_equal(clipped[:dims[0], :dims[1], :dims[2]], want["grid"])


def _with_inert_triangles(mesh, dims):
    """the mesh plus invalid (bad index, coordinate out of range), degenerate and outside triangles"""
    v, t = mesh
    n = len(v)
    extra_v = np.array([[1 << 18, 0, 0], [(1 << 18) + 1, 0, 0], [300, 300, 300], [600, 600, 600], [900, 900, 900],   # n .. n+4
                        [-900, 100, 100], [-300, 500, 100], [-600, 100, 700],                                     # n+5 .. n+7
                        [100, U * dims[1] + 1, 100], [500, U * dims[1] + 300, 100], [100, U * dims[1] + 300, 600]],  # n+8 .. n+10
                       np.int32)
    extra_t = np.array([[0, 1, n + 11], [0, n + 1, 1], [n + 2, n + 3, n + 4], [n + 2, n + 2, n + 3], [n + 5, n + 6, n + 7],
                        [n + 8, n + 9, n + 10]], np.uint32)
    return (np.concatenate([v, extra_v]), np.concatenate([extra_t[:3], t, extra_t[3:]])), (2, 2, 2)


@pytest.mark.parametrize("name", ["icosphere_80", "soup"])
def test_invalid_degenerate_and_outside_triangles_are_counted_and_inert(harness, tmp_path, name):
    mesh, dims = SMALL[name]
    more, (inv, deg, out) = _with_inert_triangles(mesh, dims)
    for modes in MODES:
        base, got = _want(name, modes), _both(more, dims, modes)
        assert np.array_equal(got["grid"], base["grid"]) and got["summary"][:3] == base["summary"][:3]
        assert got["summary"][3:] == (base["summary"][3] + 6, inv, deg, base["summary"][6] + out)
        _assert_harness(harness, tmp_path, more, dims, modes, got)


def test_quantize_vertices_rounds_half_to_even():
    import voxelengine_amd as vx
    x = np.array([[0.5 / 256, 1.5 / 256, 2.5 / 256], [-0.5 / 256, -1.5 / 256, 1.25], [3.49 / 256, 3.51 / 256, -1000.0]])
    want = [[0, 2, 2], [0, -2, 320], [3, 4, -256000]]
    assert vx.quantize_vertices(x).tolist() == want and R.quantize(x).tolist() == want
    assert vx.quantize_vertices(x).dtype == np.int32


def test_the_trap_is_armed(harness, tmp_path):
    """the harness is built so that a signed overflow aborts: the bounds of the header are checked, not assumed"""
    inp = tmp_path / "in.bin"
    inp.write_bytes(np.asarray([2, 1, 1, 1, 1, 1, 0, 0, 0], np.int32).tobytes())
    out = subprocess.run([harness, str(inp), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode != 0 and "no trap" not in out.stdout


@pytest.mark.parametrize("name", sorted(SMALL) + sorted(LARGE))
def test_host_code_equals_the_reference(harness, tmp_path, name):
    mesh, dims = {**SMALL, **LARGE}[name]
    for modes in MODES:
        want = _want(name, modes)
        on = _assert_harness(harness, tmp_path, mesh, dims, modes, want)
        if modes & R.SURFACE:  # the cull changes no bit and skips work; the items' order changes nothing
            off = _assert_harness(harness, tmp_path, mesh, dims, modes, want, cull=0)
            assert on["items"] == off["items"] and on["ballots"][0] == off["ballots"][0]
            assert on["ballots"][1] <= off["ballots"][1] and on["ballots"][2] <= off["ballots"][2]
        _assert_harness(harness, tmp_path, mesh, dims, modes, want, reverse=1)
        # the indices touched stay inside the sections the formula of the header reserves
        words, nt = (dims[0] + 31) // 32 * dims[1] * dims[2], len(mesh[1])
        assert on["top"][2] <= words and on["top"][5] <= words and on["top"][3] <= nt and on["top"][4] <= (nt + 255) // 256
        assert on["top"][3] == nt and on["top"][4] == (nt + 255) // 256


@pytest.mark.parametrize("name", ["icosphere_80", "soup", "octahedron_on_centres"])
def test_host_code_invariance_and_inert_triangles(harness, tmp_path, name):
    mesh, dims = SMALL[name]
    for modes in MODES:
        want = _want(name, modes)
        for m in _variants(mesh, 4):
            _assert_harness(harness, tmp_path, m, dims, modes, want)
        more, _ = _with_inert_triangles(mesh, dims)
        got = _assert_harness(harness, tmp_path, more, dims, modes, R.voxelize(*more, dims, modes))
        assert np.array_equal(got["grid"], want["grid"])


def test_host_code_on_empty_and_many_groups(harness, tmp_path):
    """no triangle at all; a mesh of more than two setup groups with runs of triangles that have no work item"""
    empty = (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32))
    for modes in MODES:
        got = _run_harness(harness, tmp_path, empty, (33, 4, 5), modes)
        assert not got["grid"].any() and got["summary"] == (0,) * 7 and got["items"] == 0
    v, t = R.soup(700, (40, 20, 30), 2.0, 21, margin=60)  # most triangles miss the region: whole groups without items
    for modes in MODES:
        want = R.voxelize(v, t, (40, 20, 30), modes)
        assert want["summary"][6] > 300 and want["summary"][0] > 0
        _assert_harness(harness, tmp_path, (v, t), (40, 20, 30), modes, want)


def test_the_cull_follows_the_triangle_not_its_bounding_box(harness, tmp_path):
    mesh, dims = LARGE["one_large_triangle"]
    on = _run_harness(harness, tmp_path, mesh, dims, R.SURFACE)
    off = _run_harness(harness, tmp_path, mesh, dims, R.SURFACE, cull=0)
    rows = dims[1] * dims[2] * -(-dims[0] // 64)
    assert off["ballots"][2] > 0.5 * rows  # without the cull: every row of the bounding box
    assert on["ballots"][2] < 0.2 * off["ballots"][2] and on["ballots"][2] < 3 * on["summary"][0]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_coordinate_limits(harness, tmp_path, axis):
    """vertices at +-2^18 and 1024 voxels on one axis, under the overflow trap: the closed box over the whole coordinate range
    fills every voxel, and two triangles between extreme corners equal the reference"""
    dims = coordinate_limit_dims(axis)
    box, tri = coordinate_limit_meshes()
    want = R.voxelize(*box, dims, 3)
    assert want["grid"].all()
    _assert_harness(harness, tmp_path, box, dims, 3, want)
    for modes in MODES:
        got = _assert_harness(harness, tmp_path, tri, dims, modes, R.voxelize(*tri, dims, modes))
        assert got["summary"][0] > 0


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def _layout(harness, tmp_path, dims, nt):
    raw, _ = run_harness_files(harness, tmp_path, [1, *dims, 1, 1, 0, 0, nt])
    return bool(np.frombuffer(raw[:4].tobytes(), np.uint32)[0]), int(np.frombuffer(raw[4:12].tobytes(), np.uint64)[0])


def test_voxelize_symbols_exported_and_workspace_bytes(harness, tmp_path):
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_voxelize_workspace_bytes", "vxrt_voxelize_mesh", "vxrt_voxelize_mesh_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    ws = lambda d, n: int(lib.vxrt_voxelize_workspace_bytes((C.c_int32 * 3)(*d), n))
    for bad in [(0, 8, 8), (8, -1, 8), (8, 8, 1025), (1025, 1, 1), (1 << 30, 1, 1)]:
        assert ws(bad, 10) == 0 and R.workspace_bytes(bad, 10) == 0
    assert ws((8, 8, 8), (1 << 24) + 1) == 0 and ws((8, 8, 8), 1 << 24) > 0 and ws((8, 8, 8), 0) > 0
    assert lib.vxrt_voxelize_workspace_bytes(None, 4) == 0
    for d in [(1, 1, 1), (33, 7, 5), (64, 64, 64), (1024, 1024, 1024), (1000, 3, 1024), (31, 1024, 2)]:
        for n in (0, 1, 255, 256, 257, 20480, 1 << 24):
            want = R.workspace_bytes(d, n)
            assert ws(d, n) == want > 0, (d, n)
            assert _layout(harness, tmp_path, d, n) == (True, want)
    assert _layout(harness, tmp_path, (8, 8, 8), (1 << 24) + 1) == (False, 0)
    assert ws((1024, 1024, 1024), 1 << 24) <= (1 << 27) + (1 << 26) + (1 << 20)  # the toggle bits and 4 bytes per triangle
    d3 = (C.c_int32 * 3)(8, 8, 8)
    assert lib.vxrt_voxelize_mesh(None, None, 0, None, 0, d3, 1, None, None, None, None) == -1
    assert lib.vxrt_voxelize_mesh_host(None, None, 0, None, 0, d3, 1, None, None) == -1
    assert (vx.VOX_SURFACE, vx.VOX_SOLID, vx.VOX_FRAC_BITS, vx.VOX_MAX_DIM, vx.VOX_MAX_COORD, vx.VOX_MAX_TRIANGLES) == \
        (1, 2, 8, 1024, 1 << 18, 1 << 24)
