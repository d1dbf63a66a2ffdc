"""Exact distance fields on the device (include/vxrt.h, vxrt_distance_field): the field and the summary equal to
tests/ref_dist.py on random worlds for both modes and several radii, after edits and stamps, on a bench-world window, on a
slab of one call at the 2^28-voxel limit and at the ends of int32; determinism across calls and streams; the host form;
refusals that leave the output untouched; a cleared sphere, derived by hand; and the headless example's dist line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region
from tests import ref_dist as R
from tests.helpers import eng, gen_dense, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (R.TO_SOLID, R.TO_EMPTY)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _assert_field(vx, ctx, world, origin, dims, radius, mode, stream=None, shift=(0, 0, 0)):
    """the device field against the reference computed on `world`, whose (0, 0, 0) is world voxel `shift`"""
    r = ctx.distance_field(origin, dims, radius, mode, stream=stream)
    want = R.fast(world, tuple(np.asarray(origin) - np.asarray(shift)), dims, radius, mode)
    got = r.grid()
    print("dist", origin, dims, radius, mode, tuple(r.summary), want["summary"], int((got != want["dist2"]).sum()))
    assert np.array_equal(got, want["dist2"]), (origin, dims, radius, mode)
    assert tuple(r.summary) == want["summary"], (origin, dims, radius, mode)
    return r, want


def _random(vxo, size, factor, density, seed):
    rng = np.random.default_rng(seed)
    vox = rng.random(size) < density
    vox[:, 0, :] = True
    return vxo.World.from_voxels(vox, factor), vox


@pytest.mark.parametrize("factor,size,density", [(8, (64, 64, 64), 0.08), (16, (128, 128, 128), 0.01), (32, (256, 256, 256), 0.0005)])
def test_field_equals_the_reference(eng, vxo, factor, size, density):
    vx, torch = eng
    w, vox = _random(vxo, size, factor, density, seed=factor)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        boxes = [((0, 0, 0), (size[0], 40, size[2])), ((5, 1, 7), (45, 33, 17)), ((-20, -10, -30), (61, 50, 70)),
                 ((1, 0, 2), (1, 40, 33)), ((size[0] - 40, 2, 3), (70, 20, 50))]
        for o, d in boxes:
            d = tuple(min(v, 128) for v in d)
            for mode in MODES:
                for radius in (1, 7, 32):
                    _assert_field(vx, ctx, vox, o, d, radius, mode)
    finally:
        ctx.close()


def test_radius_255_on_a_small_box(eng, vxo):
    vx, torch = eng
    w, vox = _random(vxo, (256, 256, 256), 32, 0.00002, seed=3)
    vox[:, 0, :] = False
    vox[200:, 0, :] = True
    w = vxo.World.from_voxels(vox, 32)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        for mode in MODES:
            r, want = _assert_field(vx, ctx, vox, (60, 100, 90), (40, 30, 20), 255, mode)
            if mode == R.TO_SOLID:
                assert want["summary"][3] > 32 * 32 and want["summary"][1] > 0  # values no smaller radius would give
    finally:
        ctx.close()


def test_field_follows_edits_and_stamps(eng, vxo):
    vx, torch = eng
    w, vox = _random(vxo, (128, 128, 128), 16, 0.02, seed=7)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d = (-4, 0, 3), (120, 60, 110)
        before = ctx.distance_field(o, d, 12).grid()
        rng = np.random.default_rng(8)
        ops = [(0, 0, (0, 1, 0), (127, 40, 127)), (0, 1, (30, 1, 0), (31, 6, 100)), (1, 1, (90, 10, 90), (8, 0, 0))]
        # no synchronisation between the edits and the field: the call orders after the work queued on the stream
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        stamps = [((10, 1, 10), rng.random((50, 3, 70)) < 0.2, vx.STAMP_UNION),
                  ((40, 0, 40), np.zeros((20, 1, 20), bool), vx.STAMP_REPLACE)]
        ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        vox = ref_region.apply_stamps(ref_edit.apply_edits(vox, ops), stamps)
        for mode in MODES:
            r, want = _assert_field(vx, ctx, vox, o, d, 12, mode)
            assert want["summary"][1] > 100
        assert not np.array_equal(before, ctx.distance_field(o, d, 12).grid())
    finally:
        ctx.close()


def test_cleared_sphere_leaves_its_radius_of_room(eng, vxo):
    """derived by hand, not from the reference: after a sphere of radius r around c is cleared, every voxel within r of c is
    empty, so the nearest solid voxel is further than r from c"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(np.ones((128, 128, 128), bool), 16))
        c, r = (60, 70, 50), 9
        assert ctx.distance_field(c, (1, 1, 1), 20).grid()[0, 0, 0] == 0
        ctx.edit_voxels([vx.EditSphere(c, r, 0)])
        f = ctx.distance_field((c[0] - 12, c[1] - 12, c[2] - 12), (25, 25, 25), 20)
        d2 = f.grid()
        assert r * r < d2[12, 12, 12] <= (r + 1) * (r + 1) and d2[12, 12, 12] != vx.DIST_FAR
        assert d2[12 + r, 12, 12] == 1 and d2[12 + r + 1, 12, 12] == 0 and f.summary.max_d2 == d2[12, 12, 12]
        inside = ctx.distance_field(c, (1, 1, 1), 20, vx.DIST_TO_EMPTY)
        assert inside.grid()[0, 0, 0] == 0 and inside.summary == (1, 0, 0, 0, 0)
    finally:
        ctx.close()


def _surface_y(ctx, ox, oz, below):
    """as tests/test_gpu_nav.py finds its window: the median height of a 256 x 256 patch of columns, less `below`"""
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    return max(int(np.median(heights)) - below, 0)


def test_bench_world_window(eng):
    """a 256 x 128 x 256 window of the bench world at its surface, R = 32, against the reference on read_region_host of the
    halo"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz = 4000, 3000
        o, d, radius = (ox, _surface_y(ctx, ox, oz, 48), oz), (256, 128, 256), 32
        shift = tuple(v - radius for v in o)
        world = ctx.read_region_host(shift, tuple(v + 2 * radius for v in d))  # the halo, voxel 0 at shift
        for mode in MODES:  # the reference's halo is the whole of `world`: it reads nothing beyond it
            r, want = _assert_field(vx, ctx, world, o, d, radius, mode, shift=shift)
            assert min(want["summary"][:3]) > 10000
    finally:
        ctx.close()


def test_full_limit_call(eng):
    """2^28 voxels in one call (1024 x 256 x 1024, R = 16): a 64-voxel-thick slab of it against the reference, and the
    identities zero + near + far == n and zero == the solid voxels of the box"""
    vx, torch = eng
    ctx = vx.Context(0)
    out = None
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz, radius = 3000, 4000, 16
        o, d = (ox, _surface_y(ctx, ox, oz, 128), oz), (1024, 256, 1024)
        n = d[0] * d[1] * d[2]
        assert n == 1 << 28 and ctx.distance_workspace_bytes(d, radius) > 0
        out = torch.empty(n, dtype=torch.int16, device="cuda")
        f = ctx.distance_field(o, d, radius, out=out)
        s = f.summary
        assert s.zero + s.near + s.far == n and s.max_d2 <= radius * radius
        bits = ctx.read_region(o, d)
        solid = int(np.unpackbits(bits.cpu().numpy().view(np.uint8)).sum())
        del bits
        assert s.zero == solid and s.near > 0 and s.far > 0
        z0, th = 480, 64
        slab = out.view(d[2], d[1], d[0])[z0:z0 + th].cpu().numpy().view(np.uint16).transpose(2, 1, 0)
        so, sd = (o[0], o[1], o[2] + z0), (d[0], d[1], th)
        shift = tuple(v - radius for v in so)
        world = ctx.read_region_host(shift, tuple(v + 2 * radius for v in sd))
        want = R.fast(world, (radius,) * 3, sd, radius, R.TO_SOLID)
        assert np.array_equal(slab, want["dist2"]) and want["summary"][1] > 100000
    finally:
        del out
        ctx.close()
        torch.cuda.empty_cache()


def test_boxes_at_the_ends_of_int32(eng, vxo):
    """the last origins whose halo fits in int32, far from the world: every voxel FAR for TO_SOLID, 0 for TO_EMPTY; one
    voxel further is refused"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        d, radius = (70, 9, 33), 40
        n = d[0] * d[1] * d[2]
        for k in range(3):
            for edge, step in [(INT32_MIN + radius, -1), (INT32_MAX - d[k] - radius, 1)]:
                o = [10, 10, 10]
                o[k] = edge
                f = ctx.distance_field(o, d, radius, R.TO_SOLID)
                assert (f.grid() == vx.DIST_FAR).all() and f.summary == (0, 0, n, 0, 0)
                f = ctx.distance_field(o, d, radius, R.TO_EMPTY)
                assert (f.grid() == 0).all() and f.summary == (n, 0, 0, 0, 0)
                o[k] = edge + step
                with pytest.raises(vx.VxrtError):
                    ctx.distance_field(o, d, radius)
        # a box reaching the world from far outside it
        o = (-radius - 60, 5, 5)
        _assert_field(vx, ctx, ctx.read_region_host((0, 0, 0), (128, 128, 128)), o, d, radius, R.TO_SOLID)
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams_and_host_form(eng, vxo):
    vx, torch = eng
    w, vox = _random(vxo, (256, 256, 256), 32, 0.002, seed=5)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d, radius = (-5, 0, 7), (250, 60, 230), 24
        for mode in MODES:
            first = ctx.distance_field(o, d, radius, mode)
            side = torch.cuda.Stream()
            for k in range(3):
                s = side.cuda_stream if k == 2 else None
                r = ctx.distance_field(o, d, radius, mode, stream=s)
                if s is not None:
                    side.synchronize()
                assert r.summary == first.summary and torch.equal(r.dist2, first.dist2)
            host = ctx.distance_field_host(o, d, radius, mode)
            assert np.array_equal(host.grid(), first.grid()) and host.summary == first.summary
            want = R.fast(vox, o, d, radius, mode)
            assert tuple(first.summary) == want["summary"] and np.array_equal(first.grid(), want["dist2"])
    finally:
        ctx.close()


def test_refusals_leave_the_output_untouched(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        ws = ctx.distance_workspace_bytes((8, 8, 8), 4)
        assert ws > 0
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        out = torch.full((512,), 0x1234, dtype=torch.int16, device="cuda")
        summ = torch.full((6,), 0x55, dtype=torch.int32, device="cuda")
        o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
        hout, hsum = np.full(512, 0x1234, np.uint16), np.full(6, 0x55, np.uint32)

        def field(o=o3, d=d3, r=4, m=0, wk=work.data_ptr(), ot=out.data_ptr(), s=summ.data_ptr()):
            return L.vxrt_distance_field(h, o, d, r, m, wk, ot, s, None)

        def host(o=o3, d=d3, r=4, m=0, ot=hout.ctypes.data, s=hsum.ctypes.data):
            return L.vxrt_distance_field_host(h, o, d, r, m, ot, s)

        def untouched():
            torch.cuda.synchronize()
            return bool((out == 0x1234).all()) and bool((summ == 0x55).all()) and (hout == 0x1234).all() and (hsum == 0x55).all()
        assert field() == -3 and host() == -3 and untouched()    # no world
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        for bad in [(0, 8, 8), (8, -1, 8), (1024, 1024, 257)]:
            assert field(d=(C.c_int32 * 3)(*bad)) == -1 and host(d=(C.c_int32 * 3)(*bad)) == -1
        assert field(d=(C.c_int32 * 3)(1, 1, 1 << 28), r=255) == -1       # the halo box beyond 2^36 voxels
        for bad in (0, 256, 2 ** 32 - 1):
            assert field(r=bad) == -1 and host(r=bad) == -1
        for bad in (-1, 2, 7):
            assert field(m=bad) == -1 and host(m=bad) == -1
        assert field(o=(C.c_int32 * 3)(INT32_MAX - 11, 0, 0)) == -1 and field(o=(C.c_int32 * 3)(0, INT32_MIN + 3, 0)) == -1
        assert host(o=(C.c_int32 * 3)(0, 0, INT32_MAX - 11)) == -1
        for k in ("o", "d", "wk", "ot", "s"):
            assert field(**{k: None}) == -1, k
        for k in ("o", "d", "ot", "s"):
            assert host(**{k: None}) == -1, k
        assert L.vxrt_distance_field(None, o3, d3, 4, 0, work.data_ptr(), out.data_ptr(), summ.data_ptr(), None) == -1
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert field() == -1 and host() == -1                    # a streamed world
        ctx.stream_close()
        assert untouched()
        ctx.load_world(path)
        assert field() == 0 and host() == 0 and field(o=(C.c_int32 * 3)(INT32_MAX - 12, 0, 0)) == 0
        torch.cuda.synchronize()
        assert not untouched()
    finally:
        ctx.close()


def test_headless_example_dist_line(vxo, tmp_path):
    """examples/voxelapp_headless kind 6: the printed summary equals the reference's, for both modes"""
    from oracle import vxo_edit
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    heights = np.where(vox.any(1), edge - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
    top = int(np.median(heights[40:168, 0:95]))  # the box holds the surface of its columns; it overhangs the world at z < 0
    o, d = (40, max(top - 30, 0), -5), (128, 60, 100)
    sf = tmp_path / "edits.txt"
    sf.write_text("0 6 12 %d %d %d %d %d %d\n0 6 -12 %d %d %d %d %d %d\n" % (*o, *d, *o, *d))
    out = subprocess.run([exe, str(edge), "1", str(tmp_path / "dv"), "64", "48", "1", "-", "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    want = [R.fast(vox, o, d, 12, m)["summary"] for m in MODES]
    assert want[0][1] > 1000 and want[1][1] > 1000
    line = [x for x in out.stdout.splitlines() if x.startswith("dist frame")]
    assert line == ["dist frame 0 zero %d near %d far %d max_d2 %d sum_d2 %d" % s for s in want], out.stdout
