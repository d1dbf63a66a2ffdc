"""Surface extraction on the device (include/vxrt.h, vxrt_extract_surface): quads, vertices, triangles and summary equal to
tests/ref_surface.py bit for bit -- on random worlds in both modes with box widths around a word and around a wave, at the
limits of the record's fields, across every level of the count scan, under every capacity with guard words behind it, on
every world path the region tests use, after edits, stamps and pool growth, on a bench-world window; the round trip through
vxrt_voxelize_mesh on the device; determinism; the host form; refusals in the order of the call rules; and the headless
example's surface lines (the C++ facade)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region, vxo_edit
from tests import ref_surface as R
from tests.helpers import eng, gen_dense, new_ctx, random_ops, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (R.CAP, R.OPEN)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
GUARD = 0x5A5A5A5A


def _summary(words):
    w = [int(x) for x in words]
    return (w[0], w[1], w[2], w[3], tuple(w[4:10]), tuple(w[10:16]))


def _u32(t):
    return t.cpu().numpy().view(np.uint32) if hasattr(t, "cpu") else np.asarray(t).view(np.uint32)


def _assert_equal(got, want, what):
    """an ExtractedSurface (device tensors or numpy) against a reference Surface, bit for bit"""
    s = got.summary
    print("surface", what, tuple(s), _summary(want.summary))
    assert tuple(s) == _summary(want.summary), what
    n = s.written
    assert np.array_equal(_u32(got.quads)[:n], want.quads), what
    assert np.array_equal(_u32(got.vertices)[:4 * n].view(np.int32), want.vertices), what
    assert np.array_equal(_u32(got.triangles)[:2 * n], want.triangles), what


def _assert_surface(ctx, world, origin, dims, mode, shift=(0, 0, 0), host=False):
    """the device result (and the host form's) against the reference on `world`, whose (0, 0, 0) is world voxel `shift`"""
    want = R.extract(world, tuple(int(a) - int(b) for a, b in zip(origin, shift)), dims, mode)
    got = ctx.extract_surface(origin, dims, mode, triangles=True)
    _assert_equal(got, want, (origin, dims, mode))
    if host:
        _assert_equal(ctx.extract_surface_host(origin, dims, mode, triangles=True), want, ("host", origin, dims, mode))
    return got, want


def _random(vxo, size, factor, density, seed):
    rng = np.random.default_rng(seed)
    vox = rng.random(size) < density
    return vxo.World.from_voxels(vox, factor), vox


@pytest.mark.parametrize("width", [1, 31, 32, 33, 64, 65])
def test_surface_equals_the_reference_around_words_and_waves(eng, vxo, width):
    """box widths around one 32-bit word and around the 64 lanes of a wave, origins negative and past the world's far faces;
    a dense world, so that runs cross x = 30 .. 34 and the wave boundary; device and host forms; two calls bit-identical"""
    vx, torch = eng
    w, vox = _random(vxo, (128, 64, 64), 8, 0.85, seed=width)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        for k, (o, d) in enumerate([((0, 0, 0), (width, 9, 7)), ((-1, -2, -3), (width, 11, 6)), ((128 - width // 2 - 1, 60, 59), (width, 9, 8)),
                                    ((29, 3, 5), (width, 5, 9)), ((61, 50, 1), (width, 20, 3))]):
            for mode in MODES:
                got, want = _assert_surface(ctx, vox, o, d, mode, host=k < 2)
                again = ctx.extract_surface(o, d, mode, triangles=True)
                assert again.summary == got.summary and torch.equal(again.quads, got.quads)
                assert torch.equal(again.vertices, got.vertices) and torch.equal(again.triangles, got.triangles)
        assert len(want.quads) > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [(1024, 1024, 64), (64, 1024, 1024), (1024, 64, 1024)])
def test_record_fields_at_their_limits(eng, vxo, shape):
    """fully solid bars of 1024 voxels and slabs of 1024 x 1024 in every axis pairing: w - 1 = h - 1 = 1023, coordinates up to
    1023, vertex coordinates up to 2^18"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, *shape, 8)
        ctx.edit_voxels([vx.EditBox((0, 0, 0), tuple(n - 1 for n in shape), 1)])
        thin = shape.index(64)
        boxes = [tuple(1 if k == thin else 1024 for k in range(3))]
        boxes += [tuple(1024 if k == a else 1 for k in range(3)) for a in range(3) if a != thin]
        for d in boxes:
            o = tuple(5 if k == thin else 0 for k in range(3))
            got, want = _assert_surface(ctx, np.ones(d, bool), o, d, R.CAP, shift=o)
            assert int(want.vertices.max()) == 1 << 18 and got.summary.solid == d[0] * d[1] * d[2]
        ext = want.quads[:, 1] & 0xFFFFF
        assert ext.max() == 1023 << 10 or ext.max() == 1023
        slab = R.extract(np.ones(boxes[0], bool), (0, 0, 0), boxes[0], R.CAP)
        assert (1023 | 1023 << 10) in (slab.quads[:, 1] & 0xFFFFF) and len(slab.quads) == 6
    finally:
        ctx.close()


def test_every_level_of_the_count_scan(eng, vxo):
    """92 352 rows: the scan's levels are the 64 lanes of a wave (shuffles), the 4 waves of a workgroup (256 rows, the last
    group cut short), a thread's share of the 361 groups (2 each, the last share cut short, then none) and the 256 threads
    of the group scan"""
    vx, torch = eng
    w, vox = _random(vxo, (128, 128, 128), 16, 0.5, seed=2)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d = (5, -20, 3), (96, 160, 111)
        rows = 2 * d[2] * (d[0] + 2 * d[1])
        assert rows == 92352 and rows % 256 and 256 < -(-rows // 256) < 512 and -(-rows // 256) % 2 == 1
        got, want = _assert_surface(ctx, vox, o, d, R.CAP)
        assert got.summary.quads > 1000000
    finally:
        ctx.close()


def test_capacity_and_guard_words(eng, vxo):
    """capacities 0 (NULL outputs), 1, quads - 1, quads, quads + 7: `written` and `quads` in each, the records in canonical
    order, and the guard words behind the capacity of all three buffers untouched"""
    vx, torch = eng
    w, vox = _random(vxo, (64, 64, 64), 8, 0.4, seed=9)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d = (3, -2, 30), (40, 20, 37)
        want = R.extract(vox, o, d, R.OPEN)
        n = len(want.quads)
        assert n > 1000
        L, h = ctx._L, ctx._h
        work = torch.zeros(ctx.surface_workspace_bytes(d), dtype=torch.uint8, device="cuda")
        o3, d3 = (C.c_int32 * 3)(*o), (C.c_int32 * 3)(*d)
        for cap in (0, 1, n - 1, n, n + 7):
            for tri in (True, False):
                q = torch.full((2 * cap + 8,), GUARD, dtype=torch.int32, device="cuda")
                v = torch.full((12 * cap + 8,), GUARD, dtype=torch.int32, device="cuda")
                t = torch.full((6 * cap + 8,), GUARD, dtype=torch.int32, device="cuda")
                summ = torch.zeros(16, dtype=torch.int32, device="cuda")
                rc = L.vxrt_extract_surface(h, o3, d3, R.OPEN, work.data_ptr(), q.data_ptr() if cap else None, cap,
                                            v.data_ptr() if tri and cap else None, t.data_ptr() if tri and cap else None,
                                            summ.data_ptr(), None)
                assert rc == 0
                torch.cuda.synchronize()
                cut = want.cut(cap)
                m = min(cap, n)
                assert _summary(_u32(summ)) == _summary(cut.summary), cap
                q, v, t = _u32(q), _u32(v), _u32(t)
                assert np.array_equal(q[:2 * m].reshape(-1, 2), cut.quads) and (q[2 * m:] == GUARD).all(), cap
                if tri:
                    assert np.array_equal(v[:12 * m].view(np.int32).reshape(-1, 3), cut.vertices) and (v[12 * m:] == GUARD).all(), cap
                    assert np.array_equal(t[:6 * m].reshape(-1, 3), cut.triangles) and (t[6 * m:] == GUARD).all(), cap
                else:
                    assert (v == GUARD).all() and (t == GUARD).all()
        part = ctx.extract_surface(o, d, R.OPEN, triangles=True, capacity=n - 1)
        assert part.summary.written == n - 1 and part.summary.quads == n and len(part.decode()[0]) == n - 1
    finally:
        ctx.close()


WORLDS = [  # (factor, X, Y, Z, how the world is made): the world paths of tests/test_gpu_region.py
    (8, 64, 64, 64, "upload"),
    (16, 128, 128, 128, "device"),
    (32, 256, 256, 256, "upload"),
    (8, 8192, 64, 64, "upload"),    # a wide grid: 1024 x 8 x 8 cells
    (16, 128, 128, 128, "file"),
    (32, 256, 256, 256, "edited"),   # freed slots, bricks out of cell order, a grown pool
]
BOX, SPHERE = 0, 1


@pytest.mark.parametrize("factor,X,Y,Z,how", WORLDS)
def test_surface_on_every_world_path(eng, vxo, tmp_path, factor, X, Y, Z, how):
    vx, torch = eng
    rng = np.random.default_rng(factor + X + len(how))
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx = new_ctx(vx)
    try:
        if how == "upload":
            upload(ctx, vxo.World.from_dense(dense, X, Y, Z, factor))
        elif how == "device":
            ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
        elif how == "file":
            other = new_ctx(vx)
            other.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
            other.save_world(str(tmp_path / "w.vxb"))
            other.close()
            ctx.load_world(str(tmp_path / "w.vxb"))
        else:
            ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
            n0 = ctx.world_info().nslots
            for _ in range(4):
                ops = random_ops(rng, (X, Y, Z), 24, 60)
                ctx.edit_voxels(ops)
                dense = vxo_edit.apply_edits(dense, X, Y, Z, ops)
            st = ctx.edit_voxels([(SPHERE, 1, (128, 220, 128), (30, 0, 0))])
            dense = vxo_edit.apply_edits(dense, X, Y, Z, [(SPHERE, 1, (128, 220, 128), (30, 0, 0))])
            assert st.pool_capacity > n0
        vox = vxo_edit.voxels_from_dense(dense, X, Y, Z)
        heights = np.where(vox.any(1), Y - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
        top = int(np.median(heights[:64, :64]))
        boxes = [((-3, max(top - 20, 0), -2), (70, 40, 45)), ((X - 40, max(top - 8, 0), Z - 30), (50, 33, 40))]
        if how == "edited":
            boxes.append(((95, 185, 100), (66, 70, 60)))  # the stamped sphere
        for k, (o, d) in enumerate(boxes):
            for mode in MODES:
                got, want = _assert_surface(ctx, vox, o, d, mode)
                assert k or got.summary.faces > 500
    finally:
        ctx.close()


def test_surface_follows_edits_and_stamps(eng, vxo):
    vx, torch = eng
    w, vox = _random(vxo, (128, 128, 128), 16, 0.02, seed=7)
    vox[:, 0, :] = True
    w = vxo.World.from_voxels(vox, 16)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d = (-4, 0, 3), (120, 60, 110)
        before = ctx.extract_surface(o, d).summary
        rng = np.random.default_rng(8)
        ops = [(0, 0, (0, 1, 0), (127, 40, 127)), (0, 1, (30, 1, 0), (31, 6, 100)), (1, 1, (90, 10, 90), (8, 0, 0))]
        # no synchronisation between the edits and the extraction: the call orders after the work queued on the stream
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        stamps = [((10, 1, 10), rng.random((50, 3, 70)) < 0.2, vx.STAMP_UNION),
                  ((40, 0, 40), np.zeros((20, 1, 20), bool), vx.STAMP_REPLACE)]
        ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        vox = ref_region.apply_stamps(ref_edit.apply_edits(vox, ops), stamps)
        for mode in MODES:
            got, want = _assert_surface(ctx, vox, o, d, mode)
        assert got.summary != before and got.summary.quads > 1000
    finally:
        ctx.close()


def _surface_y(ctx, ox, oz, below):
    """as tests/test_gpu_dist.py finds its window: the median height of a 256 x 256 patch of columns, less `below`"""
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    return max(int(np.median(heights)) - below, 0)


def test_bench_world_window_and_the_round_trip(eng):
    """a 128 x 128 x 128 window of the bench world at its surface against the reference on read_region_host of the halo; then
    the round trip on the device: the CAP triangles voxelized solid are the window's bits, both resident, only the
    comparison's result comes back"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz = 4000, 3000
        o, d = (ox, _surface_y(ctx, ox, oz, 64), oz), (128, 128, 128)
        shift = tuple(v - 1 for v in o)
        world = ctx.read_region_host(shift, tuple(v + 2 for v in d))  # the halo, voxel 0 at shift
        for mode in MODES:  # the reference's halo is the whole of `world`: it reads nothing beyond it
            got, want = _assert_surface(ctx, world, o, d, mode, shift=shift)
            assert want.summary[1] > 10000 and want.summary[2] < want.summary[1]
        cap = ctx.extract_surface(o, d, R.CAP, triangles=True)
        mesh = ctx.voxelize_mesh(cap.vertices, cap.triangles, d, vx.VOX_SOLID)
        bits = ctx.read_region(o, d)
        assert bool(torch.equal(mesh.bits.view(torch.int32), bits.view(torch.int32)))
        assert mesh.summary.solid == cap.summary.solid > 0 and mesh.summary.invalid == mesh.summary.degenerate == 0
    finally:
        ctx.close()


def test_round_trip_on_a_random_world(eng, vxo):
    """1 x 1 quads, whose diagonal runs through a voxel centre, and widths across a word"""
    vx, torch = eng
    w, vox = _random(vxo, (64, 64, 64), 8, 0.5, seed=4)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        side = torch.cuda.Stream()
        for o, d in [((-2, 3, 1), (67, 30, 29)), ((10, 10, 10), (33, 1, 1)), ((40, 50, 60), (30, 20, 10))]:
            cap = ctx.extract_surface(o, d, R.CAP, triangles=True, stream=side.cuda_stream)
            mesh = ctx.voxelize_mesh(cap.vertices, cap.triangles, d, vx.VOX_SOLID, stream=side.cuda_stream)
            bits = ctx.read_region(o, d, stream=side.cuda_stream)
            side.synchronize()
            assert bool(torch.equal(mesh.bits.view(torch.int32), bits.view(torch.int32))), (o, d)
            assert mesh.summary.solid == cap.summary.solid
    finally:
        ctx.close()


def test_refusals_in_order_leave_the_outputs_untouched(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        ws = ctx.surface_workspace_bytes((8, 8, 8))
        assert ws > 0 and ctx.surface_workspace_bytes((8, 8, 1025)) == 0 and ctx.surface_workspace_bytes((1024, 1024, 257)) == 0
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        quads = torch.full((4096,), 0x1234, dtype=torch.int32, device="cuda")
        verts = torch.full((4096,), 0x1234, dtype=torch.int32, device="cuda")
        tris = torch.full((4096,), 0x1234, dtype=torch.int32, device="cuda")
        summ = torch.full((16,), 0x55, dtype=torch.int32, device="cuda")
        o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
        hq, hv, ht = (np.full(4096, 0x1234, np.uint32) for _ in range(3))
        hs = np.full(16, 0x55, np.uint32)
        i3 = lambda *v: (C.c_int32 * 3)(*v)

        def call(o=o3, d=d3, m=0, wk=work.data_ptr(), q=quads.data_ptr(), cap=64, v=verts.data_ptr(), t=tris.data_ptr(),
                 s=summ.data_ptr(), ctxh=h):
            return L.vxrt_extract_surface(ctxh, o, d, m, wk, q, cap, v, t, s, None)

        def host(o=o3, d=d3, m=0, q=hq.ctypes.data, cap=64, v=hv.ctypes.data, t=ht.ctypes.data, s=hs.ctypes.data):
            return L.vxrt_extract_surface_host(h, o, d, m, q, cap, v, t, s)

        def why():
            return L.vxrt_last_error().decode()

        def untouched():
            torch.cuda.synchronize()
            dev = all(bool((x == 0x1234).all()) for x in (quads, verts, tris)) and bool((summ == 0x55).all())
            return dev and all((x == 0x1234).all() for x in (hq, hv, ht)) and (hs == 0x55).all()
        assert call() == -3 and host() == -3 and untouched()    # no world: after every argument check ...
        bad_d, bad_o = i3(8, 0, 8), i3(INT32_MIN, 0, 0)
        # ... which come in the order of the call rules: each call breaks its rule and every later one
        assert call(ctxh=None, o=None, m=7, d=bad_d) == -1 and "NULL" in why()
        for k in ("o", "d", "wk", "s"):
            assert call(**{k: None}, m=7) == -1 and "NULL" in why(), k
        for k in ("o", "d", "s"):
            assert host(**{k: None}, m=7) == -1 and "NULL" in why(), k
        for m in (-1, 2, 7):
            assert call(m=m, d=bad_d, o=bad_o, q=None, v=None) == -1 and "mode" in why()
            assert host(m=m, d=bad_d, o=bad_o, q=None, v=None) == -1 and "mode" in why()
        for bad in [(0, 8, 8), (8, -1, 8), (8, 8, 1025), (1024, 1024, 257)]:
            assert call(d=i3(*bad), o=bad_o, q=None, v=None) == -1 and "dims" in why(), bad
            assert host(d=i3(*bad), o=bad_o, q=None, v=None) == -1 and "dims" in why(), bad
        for bad in [(INT32_MIN, 0, 0), (0, INT32_MAX - 8, 0), (0, 0, INT32_MAX - 8)]:
            assert call(o=i3(*bad), q=None, v=None) == -1 and "origin" in why(), bad
            assert host(o=i3(*bad), q=None, v=None) == -1 and "origin" in why(), bad
        assert call(q=None, v=None) == -1 and "quads NULL" in why() and host(q=None, v=None) == -1 and "quads NULL" in why()
        for k in ("v", "t"):
            assert call(**{k: None}) == -1 and "both" in why() and host(**{k: None}) == -1 and "both" in why()
        assert untouched()
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        assert call(q=None, v=None) == -1 and call(t=None) == -1 and call(m=2) == -1 and call(d=bad_d) == -1 and call(o=bad_o) == -1
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert call() == -1 and host() == -1 and "streamed" in why()   # a streamed world
        ctx.stream_close()
        assert untouched()
        ctx.load_world(path)
        # the last origins whose halo fits int32, and the counting call
        assert call(o=i3(INT32_MIN + 1, 0, INT32_MAX - 9)) == 0
        torch.cuda.synchronize()
        assert bool((summ == 0).all()) and bool((quads == 0x1234).all())   # an empty box far from the world
        assert call(q=None, cap=0, v=None, t=None) == 0
        torch.cuda.synchronize()
        assert int(summ[2]) > 0 and int(summ[3]) == 0 and bool((quads == 0x1234).all())   # a counting call
        assert call() == 0 and host() == 0
        torch.cuda.synchronize()
        assert not untouched() and int(summ[3]) == min(int(summ[2]), 64) and hs[3] == min(hs[2], 64)
    finally:
        ctx.close()


def _fnv(a):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_headless_example_surface_lines(vxo, tmp_path):
    """examples/voxelapp_headless kind 8 (VoxelRaytracer3D::ExtractSurface): the printed counts equal the reference's, and the
    hashes of the facade's three vectors equal the hashes of the reference's arrays, for both modes"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    heights = np.where(vox.any(1), edge - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
    top = int(np.median(heights[40:105, 0:45]))  # the box holds the surface of its columns; it overhangs the world at z < 0
    o, d = (40, max(top - 20, 0), -5), (65, 40, 50)
    sf = tmp_path / "edits.txt"
    sf.write_text("0 8 0 %d %d %d %d %d %d\n0 8 1 %d %d %d %d %d %d\n" % (*o, *d, *o, *d))
    out = subprocess.run([exe, str(edge), "1", str(tmp_path / "dv"), "64", "48", "1", "-", "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    want = [R.extract(vox, o, d, m) for m in MODES]
    assert want[0].summary[2] > 500 and want[1].summary[1] < want[0].summary[1]
    lines = [x for x in out.stdout.splitlines() if x.startswith("surface ")]
    expect = []
    for s in want:
        expect.append("surface frame 0 solid %d faces %d quads %d tris %d" % (s.summary[0], s.summary[1], s.summary[2], 2 * len(s.quads)))
        expect.append("surface hash frame 0 quads %016x vertices %016x triangles %016x" % (_fnv(s.quads), _fnv(s.vertices), _fnv(s.triangles)))
    assert lines == expect, out.stdout
