"""Mesh voxelization and distance fields on the device at the limits of their launches (tests/launch_limit_cases.py; its
conditions are held on the CPU by tests/test_launch_limits_host.py), everything bit-equal -- words with their padding bits,
fields and summaries:

voxelization   53, 157 and 52 copies of a 1280-triangle sphere (k_vox_groups with 2 and 4 groups per thread, a partial last
               share, threads that own nothing) and 53 shuffled copies with blocks of inert triangles (shares and runs of
               groups without an item); 2^24 triangles, one more refused; rows of 1, 2, 17, 21, 22, 31 and 32 words over 35
               rows and 4096 rows of 32 words (k_vox_final's rows per wave, idle lanes and last wave); coordinates of
               +-2^18 across 1024 voxels of each axis and over a 1024 x 40 x 1024 slab.
distance       R = 32, 33, 96, 97 and 255 on a 130 x 70 x 129 box whose values are decided by targets R away along y or z
               alone, R = 255 with a target past the last tile on +y and +z; (1, 1, 2^21) voxels, whose y sweep runs in the
               second grid dimension only; boxes of 5000 voxels along x and along y."""
import ctypes as C

import numpy as np
import pytest

from oracle import vxo_edit
from tests import launch_limit_cases as L
from tests import ref_dist as RD
from tests import ref_voxelize as RV
from tests.helpers import eng, gen_dense, upload  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vox_ctx(eng):  # noqa: F811
    ctx = eng[0].Context(0)  # no world resident: a voxelization reads none
    yield ctx
    ctx.close()


def _assert_mesh(ctx, mesh, dims, modes, want):
    got = ctx.voxelize_mesh(mesh[0], mesh[1], dims, modes)
    words = got.bits.cpu().numpy().view(np.uint32)
    print("voxelize", dims, modes, len(mesh[1]), tuple(got.summary), want["summary"])
    assert tuple(got.summary) == want["summary"], (dims, modes, tuple(got.summary), want["summary"])
    assert np.array_equal(words, RV.pack(want["grid"])), (dims, modes)  # the padding bits included
    return got


def _on_device(torch, mesh):
    return torch.from_numpy(mesh[0]).cuda(), torch.from_numpy(mesh[1].view(np.int32)).cuda()


# ---- voxelization -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.MANY_GROUPS, ids=[c.name for c in L.MANY_GROUPS])
def test_many_groups(eng, vox_ctx, case):  # noqa: F811
    vx, torch = eng
    k, extra = case.shape["k"], (0, 0, 0, 0)
    if case.shape["shuffled"]:
        mesh, extra, _ = L.shuffled_copies(k)
    else:
        mesh = L.copies(k)
    dev = _on_device(torch, mesh)
    for modes in L.MODES:
        want = L.expected_copies(k, modes, extra)
        got = _assert_mesh(vox_ctx, dev, L.BASE_DIMS, modes, want)
        if k % 2 == 0:
            assert got.summary.solid == 0 and (modes != RV.SOLID or got.summary.set == 0)
        else:
            assert got.summary.set > 5000 and got.summary.triangles == len(mesh[1]) > 65536


def test_the_triangle_limit(eng, vox_ctx):  # noqa: F811
    vx, torch = eng
    nt, dims = L.TRIANGLE_LIMIT.shape["nt"], L.TRIANGLE_LIMIT.shape["dims"]
    assert nt == vx.VOX_MAX_TRIANGLES == 1 << 24
    dv, dt = _on_device(torch, L.scattered_in_degenerates(nt))
    ws = vox_ctx.voxelize_workspace_bytes(dims, nt)
    assert ws > 0 and vox_ctx.voxelize_workspace_bytes(dims, nt + 1) == 0
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    try:
        want = L.expected_copies(1, 3, (nt - 1280, 0, nt - 1280, 0))
        got = vox_ctx.voxelize_mesh(dv, dt, dims, 3, work=work)
        assert tuple(got.summary) == want["summary"] and got.summary.triangles == nt and got.summary.degenerate == nt - 1280
        assert np.array_equal(got.bits.cpu().numpy().view(np.uint32), RV.pack(want["grid"]))
        # one triangle more is refused before anything is read or written
        out = torch.full((int(got.bits.numel()),), 0x1234, dtype=torch.int32, device="cuda")
        summ = torch.full((8,), 0x55, dtype=torch.int32, device="cuda")
        rc = vox_ctx._L.vxrt_voxelize_mesh(vox_ctx._h, dv.data_ptr(), dv.numel() // 3, dt.data_ptr(), nt + 1, (C.c_int32 * 3)(*dims), 3,
                                           work.data_ptr(), out.data_ptr(), summ.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == -1 and "2^24" in vox_ctx._L.vxrt_last_error().decode()
        assert bool((out == 0x1234).all()) and bool((summ == 0x55).all())
    finally:
        del dv, dt, work
        torch.cuda.empty_cache()


@pytest.mark.parametrize("d0", L.ROW_WIDTHS + ("wide",))
def test_row_widths(eng, vox_ctx, d0):  # noqa: F811
    mesh, dims = L.row_case(d0)
    for modes in L.ROW_MODES:
        got = _assert_mesh(vox_ctx, mesh, dims, modes, L.row_reference(d0, modes))
        assert got.summary.solid > 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_coordinate_extremes(eng, vox_ctx, axis):  # noqa: F811
    dims = L.coordinate_limit_dims(axis)
    box, tri = L.coordinate_limit_meshes()
    for modes in L.MODES:
        full = _assert_mesh(vox_ctx, box, dims, modes, RV.voxelize(*box, dims, modes))
        if modes & RV.SOLID:
            assert full.summary.set == dims[0] * dims[1] * dims[2]
        assert _assert_mesh(vox_ctx, tri, dims, modes, RV.voxelize(*tri, dims, modes)).summary.set > 0


def test_coordinate_extremes_over_a_slab(eng, vox_ctx):  # noqa: F811
    tri = L.coordinate_limit_meshes()[1]
    got = _assert_mesh(vox_ctx, tri, L.EXTREME_SLAB, 3, RV.voxelize(*tri, L.EXTREME_SLAB, 3))
    assert got.summary.set > 100000 and got.summary.solid > 0 and got.summary.surface > 0


# ---- distance fields ------------------------------------------------------------------------------------------------------------
def _assert_field(ctx, origin, dims, radius, mode, want):
    r = ctx.distance_field(origin, dims, radius, mode)
    got = r.grid()
    print("dist", origin, dims, radius, mode, tuple(r.summary), want["summary"], int((got != want["dist2"]).sum()))
    assert np.array_equal(got, want["dist2"]), (origin, dims, radius, mode)
    assert tuple(r.summary) == want["summary"], (origin, dims, radius, mode)
    return got


@pytest.mark.parametrize("mode", L.DIST_MODES)
@pytest.mark.parametrize("group", list(L.RADIUS_GROUPS))
def test_each_instantiation_at_its_first_and_last_radius(eng, vxo, group, mode):  # noqa: F811
    vx, torch = eng
    shape, origin, targets = L.radius_case(group, mode)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_dense(L.dense_world(shape, mode == RD.TO_EMPTY, targets), *shape, 16))
        fields = {}
        for R in L.RADIUS_GROUPS[group]:
            want = L.radius_reference(group, R, mode)
            assert want["summary"][2] > 0 and want["summary"][3] == R * R
            fields[R] = _assert_field(ctx, origin, L.RADIUS_BOX, R, mode, want)
        if len(fields) == 2:  # wherever the smaller radius gives a value, the larger one gives the same
            a, b = (fields[R] for R in L.RADIUS_GROUPS[group])
            assert np.array_equal(a[a != RD.FAR], b[a != RD.FAR])
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", L.DIST_MODES)
def test_y_sweep_in_the_second_grid_dimension(eng, vxo, mode):  # noqa: F811
    vx, torch = eng
    s = L.SECOND_GRID.shape
    world = L.long_z_world()
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(world, 8))
        want = RD.fast(world, s["origin"], s["dims"], s["radius"], mode)
        assert want["summary"][1] > 0  # near: values only the workgroups with blockIdx.y > 0 compute
        if mode == RD.TO_SOLID:
            assert want["summary"][2] >= -s["origin"][2]
        _assert_field(ctx, s["origin"], s["dims"], s["radius"], mode, want)
    finally:
        ctx.close()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", L.DIST_MODES)
@pytest.mark.parametrize("case", L.LONG_CASES, ids=[c.name for c in L.LONG_CASES])
def test_boxes_of_5000_voxels(eng, vxo, case, mode):  # noqa: F811
    vx, torch = eng
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_INT_TERRAIN, 128, 128, 128), 128, 128, 128)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        o, d = case.shape["origin"], case.shape["dims"]
        want = RD.fast(vox, o, d, L.LONG_RADIUS, mode)
        assert want["summary"][1] > 0 and (mode == RD.TO_EMPTY or want["summary"][2] > 4000)
        _assert_field(ctx, o, d, L.LONG_RADIUS, mode, want)
    finally:
        ctx.close()
