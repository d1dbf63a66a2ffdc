"""GPU checks of mesh voxelization (include/vxrt.h, vxrt_voxelize_mesh): bits and summary bit-equal to tests/ref_voxelize.py
for every generator in every mode -- meshes partly and wholly outside the region, negative coordinates, row widths that are not
multiples of 32 -- soups of 10^4 triangles, one triangle across 512^3, a 20 480-triangle sphere in 448^3; determinism across
calls and streams, the host form, refusals that leave the outputs untouched, no world resident; and the composition with
stamps, the brickmap tables, a rendered frame, floating islands and the headless example's mesh line.  The reference is the
fast pair of tests/ref_voxelize.py; tests/test_voxelize_host.py holds it to the slow restatements, and here the generator
cases also assert the solid field against the per-voxel sign form (the larger cases would take minutes in it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ref_voxelize as R
from tests.helpers import assert_frames, assert_tables, eng, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (R.SURFACE, R.SOLID, R.SURFACE | R.SOLID)
U = R.UNIT


def _assert_mesh(vx, ctx, mesh, dims, modes, want=None, **kw):
    want = want or R.voxelize(*mesh, dims, modes)
    got = ctx.voxelize_mesh(mesh[0], mesh[1], dims, modes, **kw)
    words = got.bits.cpu().numpy().view(np.uint32)
    assert tuple(got.summary) == want["summary"], (dims, modes, tuple(got.summary), want["summary"])
    assert np.array_equal(words, R.pack(want["grid"])), (dims, modes)  # the padding bits included
    assert np.array_equal(got.grid(), want["grid"])
    return got


GENERATORS = {
    "box": (lambda: R.box_mesh((131, 377, 201), (9711, 5403, 7999)), (45, 30, 37)),
    "box_partly_outside": (lambda: R.box_mesh((-5000, 300, -77), (15000, 50000, 900)), (70, 33, 5)),
    "octahedron": (lambda: R.octahedron((20 * U + 128, 17 * U + 128, 15 * U + 128), 13 * U), (41, 35, 33)),
    "octahedron_negative": (lambda: R.octahedron((-700, 3000, -2000), 9000), (31, 40, 37)),
    "icosphere": (lambda: R.icosphere((30.2, 28.7, 31.4), 25.3, 3), (63, 60, 65)),
    "icosphere_off_the_corner": (lambda: R.icosphere((70.0, -4.0, 66.0), 25.0, 2), (65, 31, 64)),
    "torus": (lambda: R.torus((50.0, 12.5, 44.0), 33.0, 9.3, 48, 20), (100, 25, 90)),
    "heightfield": (lambda: R.heightfield(16, 12, 8.0, 20.0, 7), (129, 22, 97)),
    "soup": (lambda: R.soup(800, (97, 33, 40), 3.0, 8), (97, 33, 40)),
    "wholly_outside": (lambda: R.icosphere((-40.0, 10.0, 10.0), 12.0, 1), (33, 20, 20)),
    "wholly_beyond_x": (lambda: R.icosphere((80.0, 10.0, 10.0), 8.0, 1), (33, 20, 20)),
}


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_every_generator_equals_the_reference(eng, name):
    vx, torch = eng
    make, dims = GENERATORS[name]
    mesh = make()
    ctx = vx.Context(0)  # no world resident
    try:
        for modes in MODES:
            want = R.voxelize(*mesh, dims, modes)
            if modes == R.SOLID:
                assert np.array_equal(want["grid"], R.solid_sign(*mesh, dims))
            got = _assert_mesh(vx, ctx, mesh, dims, modes, want)
            if name.startswith("wholly"):
                assert got.summary.set == 0 and got.summary.outside == got.summary.triangles
            else:
                assert got.summary.set > 0
    finally:
        ctx.close()


def test_hand_derived_box_fill_and_inert_triangles(eng):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        for a, b, dims in [((U + 128,) * 3, (5 * U + 128, 4 * U + 128, 6 * U + 128), (8, 7, 9)), ((2 * U, U, 3 * U), (6 * U, 5 * U, 7 * U), (9, 8, 8)),
                           ((-3000, -3000, -3000), (90000, 90000, 90000), (65, 4, 3))]:
            g = ctx.voxelize_mesh(*R.box_mesh(a, b), dims, R.SOLID).grid()
            m = [(U * np.arange(d) + 128 >= lo) & (U * np.arange(d) + 128 < hi) for d, lo, hi in zip(dims, a, b)]
            assert np.array_equal(g, m[0][:, None, None] & m[1][None, :, None] & m[2][None, None, :])
        v, t = R.icosphere((10.0, 9.0, 11.0), 7.5, 2)
        n = len(v)
        v2 = np.concatenate([v, np.array([[(1 << 18) + 1, 0, 0], [300, 300, 300], [600, 600, 600], [900, 900, 900]], np.int32)])
        t2 = np.concatenate([np.array([[0, 1, n + 4], [0, n, 1]], np.uint32), t, np.array([[n + 1, n + 2, n + 3]], np.uint32)])
        for modes in MODES:
            base = R.voxelize(v, t, (21, 19, 22), modes)
            got = _assert_mesh(vx, ctx, (v2, t2), (21, 19, 22), modes)
            assert np.array_equal(got.grid(), base["grid"]) and tuple(got.summary)[3:6] == (len(t) + 3, 2, 1)
    finally:
        ctx.close()


def test_soup_of_ten_thousand_small_triangles(eng):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        for dims, size, seed in [((160, 100, 130), 1.5, 1), ((95, 64, 257), 4.0, 2)]:
            mesh = R.soup(10000, dims, size, seed)
            for modes in MODES:
                assert _assert_mesh(vx, ctx, mesh, dims, modes).summary.set > 5000
    finally:
        ctx.close()


def test_one_large_triangle_across_512_cubed(eng):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        v = np.array([[-900, -700, 40000], [131000, 20000, 131500], [60000, 131072, -300]], np.int32)
        mesh = (v, np.array([[0, 1, 2]], np.uint32))
        for modes in MODES:
            got = _assert_mesh(vx, ctx, mesh, (512, 512, 512), modes)
            assert got.summary.set > 100000
    finally:
        ctx.close()


def test_icosphere_of_20480_triangles_in_448_cubed(eng):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        mesh = R.icosphere((224.0, 224.0, 224.0), 200.0, 5)
        assert len(mesh[1]) == 20480
        dims = (448, 448, 448)
        counts = R.triangles(*mesh, dims)[1]
        fields = {R.SURFACE: R.surface_sat(*mesh, dims), R.SOLID: R.solid_threshold(*mesh, dims)}
        fields[3] = fields[R.SURFACE] | fields[R.SOLID]
        got = {}
        for modes in MODES:  # each mode bit-equal to its own reference field
            ns, nf = int(fields[R.SURFACE].sum()) * (modes & 1), int(fields[R.SOLID].sum()) * (modes >> 1)
            want = {"grid": fields[modes], "summary": (int(fields[modes].sum()), ns, nf) + counts}
            got[modes] = _assert_mesh(vx, ctx, mesh, dims, modes, want)
        ball = 4.0 / 3.0 * np.pi * 200.0 ** 3
        assert abs(got[3].summary.solid - ball) < 0.01 * ball
        surface_only, solid_only, got = got[R.SURFACE], got[R.SOLID], got[3]
        assert torch.equal(surface_only.bits | solid_only.bits, got.bits)
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams_and_host_form(eng):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        mesh, dims = R.torus((50.0, 12.5, 44.0), 33.0, 9.3, 48, 20), (100, 25, 90)
        dv = torch.from_numpy(mesh[0]).cuda()
        dt = torch.from_numpy(mesh[1].view(np.int32)).cuda()
        torch.cuda.synchronize()
        for modes in MODES:
            first = ctx.voxelize_mesh(dv, dt, dims, modes)
            side = torch.cuda.Stream()
            ws = ctx.voxelize_workspace_bytes(dims, len(mesh[1]))
            work = torch.empty(ws, dtype=torch.uint8, device="cuda")
            for k in range(4):
                s = side.cuda_stream if k >= 2 else None
                r = ctx.voxelize_mesh(dv, dt, dims, modes, stream=s, work=work if k % 2 else None)
                if s is not None:
                    side.synchronize()
                assert r.summary == first.summary and torch.equal(r.bits, first.bits)
                torch.cuda.synchronize()
            host = ctx.voxelize_mesh_host(mesh[0], mesh[1], dims, modes)
            assert np.array_equal(host.grid(), first.grid()) and host.summary == first.summary
            want = R.voxelize(*mesh, dims, modes)
            assert tuple(first.summary) == want["summary"] and np.array_equal(first.grid(), want["grid"])
    finally:
        ctx.close()


def test_refusals_leave_the_output_untouched_and_no_triangle_is_valid(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        mesh = R.octahedron((1000, 1000, 1000), 700)
        dv, dt = torch.from_numpy(mesh[0]).cuda(), torch.from_numpy(mesh[1].view(np.int32)).cuda()
        ws = ctx.voxelize_workspace_bytes((8, 8, 8), 8)
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        out = torch.full((64,), 0x1234, dtype=torch.int32, device="cuda")
        summ = torch.full((8,), 0x55, dtype=torch.int32, device="cuda")
        hout, hsum = np.full(64, 0x1234, np.uint32), np.full(8, 0x55, np.uint32)
        d3 = (C.c_int32 * 3)(8, 8, 8)

        def dev(v=dv.data_ptr(), nv=6, t=dt.data_ptr(), nt=8, d=d3, m=3, wk=work.data_ptr(), ot=out.data_ptr(), s=summ.data_ptr()):
            return L.vxrt_voxelize_mesh(h, v, nv, t, nt, d, m, wk, ot, s, None)

        def host(v=mesh[0].ctypes.data, nv=6, t=mesh[1].ctypes.data, nt=8, d=d3, m=3, ot=hout.ctypes.data, s=hsum.ctypes.data):
            return L.vxrt_voxelize_mesh_host(h, v, nv, t, nt, d, m, ot, s)

        def untouched():
            torch.cuda.synchronize()
            return bool((out == 0x1234).all()) and bool((summ == 0x55).all()) and (hout == 0x1234).all() and (hsum == 0x55).all()
        for bad in [(0, 8, 8), (8, -1, 8), (8, 8, 1025)]:
            assert dev(d=(C.c_int32 * 3)(*bad)) == -1 and host(d=(C.c_int32 * 3)(*bad)) == -1
        for bad in (0, 4, -1, 7):
            assert dev(m=bad) == -1 and host(m=bad) == -1
        assert dev(nt=(1 << 24) + 1) == -1 and host(nt=(1 << 24) + 1) == -1
        for k in ("v", "t", "d", "wk", "ot", "s"):
            assert dev(**{k: None}) == -1, k
        for k in ("v", "t", "d", "ot", "s"):
            assert host(**{k: None}) == -1, k
        assert L.vxrt_voxelize_mesh(None, dv.data_ptr(), 6, dt.data_ptr(), 8, d3, 3, work.data_ptr(), out.data_ptr(), summ.data_ptr(), None) == -1
        # the order of the checks: the modes before the dims, the dims before the triangle count, the count before the mesh
        msg = lambda: L.vxrt_last_error().decode()
        assert dev(m=0, d=(C.c_int32 * 3)(0, 8, 8), nt=1 << 25, v=None) == -1 and "modes" in msg()
        assert dev(d=(C.c_int32 * 3)(0, 8, 8), nt=1 << 25, v=None) == -1 and "dims" in msg()
        assert dev(nt=1 << 25, v=None) == -1 and "2^24" in msg()
        assert dev(v=None) == -1 and "NULL" in msg()
        assert untouched()
        # no triangle: valid, zeroed bits and summary, the mesh pointers may be NULL; no world is resident in this context
        assert dev(v=None, t=None, nt=0) == 0 and host(v=None, t=None, nt=0) == 0
        torch.cuda.synchronize()
        assert bool((out == 0).all()) and bool((summ == 0).all()) and (hout == 0).all() and (hsum == 0).all()
        out.fill_(0x1234)
        assert dev() == 0 and host() == 0
        torch.cuda.synchronize()
        want = R.voxelize(*mesh, (8, 8, 8), 3)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.pack(want["grid"])) and np.array_equal(hout, R.pack(want["grid"]))
        assert tuple(int(x) for x in summ.cpu().numpy()[:7]) == want["summary"] == tuple(int(x) for x in hsum[:7])
        # a streamed world does not matter either
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        out.fill_(0)
        assert dev() == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.pack(want["grid"]))
        ctx.stream_close()
    finally:
        ctx.close()


def test_strided_out_and_work_are_refused_and_left_unchanged(eng):
    """voxelize_mesh hands the library the tensors' addresses as dense buffers: a tensor with a stride is refused before
    the library is called, and the dense part of the same memory is accepted"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        mesh, dims = R.octahedron((1000, 1000, 1000), 700), (8, 8, 8)
        n = vx.region_words(dims)
        ws = ctx.voxelize_workspace_bytes(dims, len(mesh[1]))
        out = torch.full((2 * n,), 0x1234, dtype=torch.int32, device="cuda")
        work = torch.full((2 * ws,), 0xA5, dtype=torch.uint8, device="cuda")
        for kw in (dict(out=out[::2]), dict(work=work[::2]), dict(out=out[::2], work=work[::2])):
            with pytest.raises(ValueError):
                ctx.voxelize_mesh(mesh[0], mesh[1], dims, 3, **kw)
        torch.cuda.synchronize()
        assert bool((out == 0x1234).all()) and bool((work == 0xA5).all())
        got = ctx.voxelize_mesh(mesh[0], mesh[1], dims, 3, out=out[:n], work=work[:ws])
        want = R.voxelize(*mesh, dims, 3)
        assert np.array_equal(got.grid(), want["grid"]) and tuple(got.summary) == want["summary"]
        assert bool((out[n:] == 0x1234).all()) and bool((work[ws:] == 0xA5).all())
    finally:
        ctx.close()


# ---- composition with the resident world --------------------------------------------------------------------------------------
def _bbox(mesh):
    v = mesh[0].astype(np.int64)
    lo, hi = (v.min(0) - 1) >> 8, v.max(0) >> 8
    return lo, tuple(int(x) for x in hi - lo + 1)


def _combine(old, grid, at, mode):
    """the world after a stamp of `grid` at `at` in `mode`, clipped to the world"""
    new = old.copy()
    lo = [max(a, 0) for a in at]
    hi = [min(a + d, s) for a, d, s in zip(at, grid.shape, old.shape)]
    if any(l >= h for l, h in zip(lo, hi)):
        return new
    w = tuple(slice(l, h) for l, h in zip(lo, hi))
    g = grid[tuple(slice(l - a, h - a) for l, h, a in zip(lo, hi, at))]
    new[w] = g if mode == 0 else (new[w] | g if mode == 1 else new[w] & ~g)
    return new


@pytest.mark.parametrize("stamp_mode", [0, 1, 2])
def test_stamp_mesh_into_a_random_world(eng, vxo, stamp_mode):
    vx, torch = eng
    rng = np.random.default_rng(30 + stamp_mode)
    vox = rng.random((128, 64, 128)) < 0.3
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        mesh = R.icosphere((3.3, 2.1, -1.7), 21.5, 3)   # mesh units around its own origin
        lo, dims = _bbox(mesh)
        for origin in [(60, 30, 64), (5, 50, 120)]:     # inside the world; overhanging three faces
            m, st, at = ctx.stamp_mesh(mesh[0], mesh[1], origin, 3, stamp_mode)
            assert at == tuple(int(o + l) for o, l in zip(origin, lo)) and m.dims == dims
            want = R.voxelize(mesh[0] - U * lo.astype(np.int32), mesh[1], dims, 3)
            assert np.array_equal(m.grid(), want["grid"]) and tuple(m.summary) == want["summary"]
            vox = _combine(vox, want["grid"], at, stamp_mode)
            assert np.array_equal(ctx.read_region_host((0, 0, 0), vox.shape), vox)
            assert st.bricks_touched > 0
        w = vxo.World.from_voxels(vox, 8)
        assert_tables(ctx, w)
        if stamp_mode == 1:
            assert_frames(vx, ctx, torch, vxo, w, cams="A", variants=(4,))
    finally:
        ctx.close()


def test_stamped_models_and_floating_islands(eng, vxo):
    vx, torch = eng
    vox = np.zeros((128, 128, 128), bool)
    vox[:, :8, :] = True  # a floor
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        model = R.box_mesh((0, 0, 0), (20 * U, 30 * U, 16 * U))
        ball = R.icosphere((0.0, 0.0, 0.0), 11.0, 2)
        ctx.stamp_mesh(*model, (40, 8, 50), R.SOLID, vx.STAMP_UNION)       # stands on the floor
        isl = ctx.find_islands((0, 0, 0), (128, 128, 128), anchors=vx.ISLAND_ANCHOR_FLOOR)
        assert isl.summary.islands == 0 and isl.summary.components == 1
        m, _, at = ctx.stamp_mesh(*ball, (90, 70, 60), R.SOLID, vx.STAMP_UNION)  # in mid-air
        isl = ctx.find_islands((0, 0, 0), (128, 128, 128), anchors=vx.ISLAND_ANCHOR_FLOOR)
        assert isl.summary.islands == 1 and isl.summary.components == 2 and isl.summary.island_voxels == m.summary.set
        assert all(int(l) >= a for l, a in zip(isl.table[0]["lo"], at)) and isl.table[0]["voxels"] == m.summary.solid
    finally:
        ctx.close()


def test_headless_example_mesh_line(vxo, tmp_path):
    """examples/voxelapp_headless kind 7: the printed counts equal the reference's, for the three modes"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    sf = tmp_path / "edits.txt"
    sf.write_text("0 7 1 100 200 90 9 0 0\n0 7 2 40 210 60 14 0 0\n0 7 3 250 128 3 20 0 0\n")
    out = subprocess.run([exe, "256", "1", str(tmp_path / "dv"), "64", "48", "1", "-", "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [x for x in out.stdout.splitlines() if x.startswith("mesh before frame")]
    assert len(lines) == 3, out.stdout
    from oracle import vxo_edit
    from tests.helpers import gen_dense
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, 256, 256, 256), 256, 256, 256)
    bricks = lambda v: v.reshape(8, 32, 8, 32, 8, 32).any(axis=(1, 3, 5))  # the example's world has 32-voxel bricks
    for line, (modes, r, a) in zip(lines, [(1, 9, (100, 200, 90)), (2, 14, (40, 210, 60)), (3, 20, (250, 128, 3))]):
        mesh = R.octahedron((128, 128, 128), U * r)
        lo, dims = _bbox(mesh)
        want = R.voxelize(mesh[0] - U * lo.astype(np.int32), mesh[1], dims, modes)
        at = [int(o + l) for o, l in zip(a, lo)]
        after = _combine(vox, want["grid"], at, 1)
        # touched: the bricks of the stamp's box clipped to the world; created: those empty before and not after
        span = [(max(o, 0) >> 5, (min(o + d, 256) - 1) >> 5) for o, d in zip(at, dims)]
        touched = int(np.prod([h - l + 1 for l, h in span]))
        created = int((bricks(after) & ~bricks(vox)).sum())
        assert line == "mesh before frame 0: 8 triangles, %d set voxels, %d bricks touched, %d created" % \
            (want["summary"][0], touched, created), (line, want["summary"])
        assert want["summary"][0] > 100
        vox = after
