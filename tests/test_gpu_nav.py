"""Navigation fields on the device (include/vxrt.h, vxrt_nav_field / vxrt_nav_paths): walkable bits, dist, next and summary
equal to tests/ref_nav.py on random worlds for five agents, after edits and stamps, on a bench-world window; paths equal to
the reference's decoding with every status; determinism across calls and streams; refusals; the work following the frontier
on a snake corridor of more than 1000 levels; and the headless example's nav line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region
from tests import ref_nav as R
from tests.helpers import eng, gen_dense, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGENTS = [(1, 2, 1, 3), (2, 3, 0, 1), (1, 1, 2, 8), (3, 2, 1, 2), (8, 32, 8, 32)]


def _grid(t, dims, dtype):
    return t.cpu().numpy().view(dtype).reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)


def _want(world, origin, dims, agent, goals, max_dist=1 << 24):
    if R.have_scipy():
        return R.nav_field_scipy(world, origin, dims, agent, goals, max_dist)
    return R.nav_field(world, origin, dims, agent, goals, max_dist)


def _assert_field(vx, ctx, world, origin, dims, agent, goals, max_dist=1 << 24, stream=None, shift=(0, 0, 0)):
    """the device field against the reference computed on `world`, whose (0, 0, 0) is world cell `shift`"""
    r = ctx.nav_field(origin, dims, goals, vx.NavAgent(*agent), max_dist, dist=True, stream=stream)
    sh = np.asarray(shift)
    want = _want(world, tuple(np.asarray(origin) - sh), dims, agent, [tuple(np.asarray(g) - sh) for g in goals], max_dist)
    assert tuple(r.summary)[:6] == want["summary"], (origin, dims, agent)
    tiles = (dims[0] + 31) // 32 * ((dims[1] + 15) // 16) * ((dims[2] + 15) // 16)
    assert r.summary.tiles_total == tiles
    assert np.array_equal(r.walkable.cpu().numpy().view(np.uint32), vx.pack_region(want["walkable"]))
    assert np.array_equal(_grid(r.dist, dims, np.uint32), want["dist"])
    assert np.array_equal(_grid(r.next, dims, np.uint8), want["next"])
    return r, want


def _nodes(want, origin, n, rng):
    p = np.argwhere(want["walkable"])
    if len(p) == 0:
        return []
    return [tuple(int(v) for v in p[i] + np.asarray(origin)) for i in rng.choice(len(p), min(n, len(p)), replace=False)]


def _random(vxo, size, factor, density, seed):
    rng = np.random.default_rng(seed)
    vox = rng.random(size) < density
    vox[:, 0, :] = True
    return vxo.World.from_voxels(vox, factor), vox


@pytest.mark.parametrize("factor,size,density", [(8, (64, 64, 64), 0.08), (16, (128, 128, 128), 0.15), (32, (256, 256, 256), 0.03)])
def test_field_equals_the_reference(eng, vxo, factor, size, density):
    vx, torch = eng
    w, vox = _random(vxo, size, factor, density, seed=factor)
    rng = np.random.default_rng(factor + 1)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        boxes = [((0, 0, 0), (size[0], 40, size[2])), ((5, 1, 7), (45, 33, 17)), ((-20, -10, -30), (61, 50, 70)),
                 ((1, 0, 2), (1, 40, 33)), ((size[0] - 40, 2, 3), (70, 20, 50))]
        for i, (o, d) in enumerate(boxes):
            d = tuple(min(v, 128) for v in d)
            for agent in AGENTS:
                probe = R.nav_field(vox, o, d, agent, [])
                goals = _nodes(probe, o, 1 + 3 * i, rng) + [(o[0], o[1] + d[1] + 5, o[2])]
                _assert_field(vx, ctx, vox, o, d, agent, goals, 1 << 24 if i % 2 == 0 else 9)
    finally:
        ctx.close()


def test_field_follows_edits_and_stamps(eng, vxo):
    vx, torch = eng
    w, vox = _random(vxo, (128, 128, 128), 16, 0.1, seed=7)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d = (0, 0, 0), (128, 48, 128)
        before = ctx.nav_field(o, d, [(60, 1, 60)], vx.NavAgent())
        rng = np.random.default_rng(8)
        ops = [(0, 0, (0, 1, 0), (127, 40, 127)), (0, 1, (30, 1, 0), (31, 6, 100)), (1, 1, (90, 10, 90), (8, 0, 0))]
        # no synchronisation between the edits and the field: the call orders after the work queued on the stream
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        stamps = [((10, 1, 10), rng.random((50, 3, 70)) < 0.2, vx.STAMP_UNION),
                  ((40, 0, 40), np.zeros((20, 1, 20), bool), vx.STAMP_REPLACE)]
        ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        vox = ref_region.apply_stamps(ref_edit.apply_edits(vox, ops), stamps)
        for agent in AGENTS[:4]:
            r, want = _assert_field(vx, ctx, vox, o, d, agent, [(60, 1, 60), (5, 1, 120)])
            assert want["summary"][3] > 100
        assert not torch.equal(before.next, ctx.nav_field(o, d, [(60, 1, 60)], vx.NavAgent()).next)
        box = ctx.read_region_host((0, 0, 0), (128, 128, 128))
        assert np.array_equal(box, vox)
    finally:
        ctx.close()


def test_bench_world_window(eng):
    """a 256 x 64 x 256 window of the bench world at its surface, against the reference on read_region_host"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz = 4000, 3000
        col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
        heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
        y0 = max(int(np.median(heights)) - 24, 0)
        o, d = (ox, y0, oz), (256, 64, 256)
        shift = (ox, y0 - 1, oz)
        world = ctx.read_region_host(shift, (256 + 7, 64 + 32, 256 + 7))  # the halo of every agent below, cell 0 at shift
        rng = np.random.default_rng(1)
        for agent in [(1, 2, 1, 3), (2, 3, 2, 4)]:
            probe = R.nav_field(world, (0, 1, 0), d, agent, [])
            goals = _nodes(probe, o, 1, rng)
            r, want = _assert_field(vx, ctx, world, o, d, agent, goals, shift=shift)
            assert want["summary"][0] > 10000 and want["summary"][3] > 1000
    finally:
        ctx.close()


def test_paths_equal_the_decoding(eng, vxo):
    vx, torch = eng
    w, vox = _random(vxo, (64, 64, 64), 8, 0.06, seed=21)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d, agent = (0, 0, 0), (64, 24, 64), (1, 2, 1, 3)
        probe = R.nav_field(vox, o, d, agent, [])
        rng = np.random.default_rng(22)
        goals = _nodes(probe, o, 2, rng)
        r, want = _assert_field(vx, ctx, vox, o, d, agent, goals)
        nodes = np.argwhere(want["walkable"])
        starts = np.concatenate([nodes[rng.integers(0, len(nodes), 3000)],
                                 np.stack([rng.integers(-3, 67, 1000), rng.integers(-3, 27, 1000), rng.integers(-3, 67, 1000)], 1),
                                 np.asarray(goals)]).astype(np.int32)
        for max_steps, cells in [(0, True), (7, True), (200, True), (200, False)]:
            p = r.paths(starts, max_steps, cells=cells)
            c, l, st = R.decode_paths(want["next"], o, agent, starts, max_steps)
            assert np.array_equal(p.lengths.cpu().numpy(), l) and np.array_equal(p.status.cpu().numpy(), st)
            if cells:
                assert np.array_equal(p.cells.cpu().numpy(), c)
            if max_steps == 7:
                assert set(st.tolist()) == {R.AT_GOAL, R.NO_PATH, R.TRUNCATED, R.OUTSIDE}
        empty = r.paths(np.zeros((0, 3), np.int32), 5)
        assert empty.lengths.numel() == 0
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams(eng, vxo):
    vx, torch = eng
    w, vox = _random(vxo, (256, 256, 256), 32, 0.05, seed=5)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d = (-5, 0, 7), (250, 60, 230)
        goals = [(100, 1, 100), (3, 1, 200), (200, 1, 5)]
        first = ctx.nav_field(o, d, goals, vx.NavAgent(2, 2, 1, 2))
        side = torch.cuda.Stream()
        for k in range(3):
            s = side.cuda_stream if k == 2 else None
            r = ctx.nav_field(o, d, goals, vx.NavAgent(2, 2, 1, 2), stream=s)
            assert torch.equal(r.walkable, first.walkable) and torch.equal(r.next, first.next) and torch.equal(r.dist, first.dist)
            assert r.summary == first.summary
        no_dist = ctx.nav_field(o, d, goals, vx.NavAgent(2, 2, 1, 2), dist=False)
        assert no_dist.dist is None and torch.equal(no_dist.next, first.next) and no_dist.summary == first.summary
        host = ctx.nav_field_host(o, d, goals, vx.NavAgent(2, 2, 1, 2))
        assert np.array_equal(host.next, _grid(first.next, d, np.uint8)) and host.summary == first.summary
        assert np.array_equal(host.dist, _grid(first.dist, d, np.uint32))
        assert np.array_equal(vx.pack_region(host.walkable), first.walkable.cpu().numpy().view(np.uint32))
        want = _want(vox, o, d, (2, 2, 1, 2), goals)
        assert tuple(first.summary)[:6] == want["summary"]
    finally:
        ctx.close()


def test_snake_corridor_work_follows_the_frontier(eng, vxo):
    vx, torch = eng
    snake = R.snake_world(256, 128)
    vox = np.zeros((256, 64, 128), bool)
    vox[:, :snake.shape[1]] = snake
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        r, want = _assert_field(vx, ctx, vox, (0, 0, 0), snake.shape, (1, 2, 1, 3), [(0, 1, 0)])
        s = r.summary
        assert s.levels > 1000 and s.tile_visits <= s.levels * s.tiles_total / 16, s
        cut = ctx.nav_field((0, 0, 0), snake.shape, [(0, 1, 0)], vx.NavAgent(), max_dist=500)
        assert cut.summary.max_dist_found == 500 and cut.summary.levels == 501
        assert cut.summary.tile_visits <= 501 * cut.summary.tiles_total / 16
    finally:
        ctx.close()


def test_refusals(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        buf = torch.zeros(1 << 20, dtype=torch.int32, device="cuda")
        p = buf.data_ptr()                       # workspace
        wk, nx, sp = p + (1 << 21), p + (1 << 21) + (1 << 18), p + (1 << 21) + (1 << 19)
        gl = torch.tensor([[1, 1, 1]], dtype=torch.int32, device="cuda")
        o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
        ag = vx.NavAgent()._c()
        hw, hn, hs = np.zeros(1 << 12, np.uint32), np.zeros(1 << 12, np.uint8), np.zeros(8, np.uint32)

        def field(o=o3, d=d3, a=ag, g=gl.data_ptr(), n=1, md=10, work=p, walk=wk, nxt=nx, s=sp):
            return L.vxrt_nav_field(h, o, d, a, g, n, md, work, walk, nxt, None, s, None)

        def host(o=o3, d=d3, a=ag, g=np.ones(3, np.int32), n=1, md=10):
            return L.vxrt_nav_field_host(h, o, d, a, g.ctypes.data if g is not None else None, n, md, hw.ctypes.data,
                                         hn.ctypes.data, None, hs.ctypes.data)
        assert field() == -3 and host() == -3     # no world
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        for bad in [(0, 8, 8), (8, -1, 8), (1024, 1024, 257)]:
            assert field(d=(C.c_int32 * 3)(*bad)) == -1
        assert field(o=(C.c_int32 * 3)(2 ** 31 - 4, 0, 0)) == -1
        for bad in [(0, 2, 1, 3), (9, 2, 1, 3), (1, 0, 1, 3), (1, 33, 1, 3), (1, 2, -1, 3), (1, 2, 9, 3), (1, 2, 1, -1), (1, 2, 1, 33)]:
            assert field(a=(C.c_int32 * 4)(*bad)) == -1 and host(a=(C.c_int32 * 4)(*bad)) == -1
        assert field(md=0) == -1 and field(md=(1 << 24) + 1) == -1 and host(md=0) == -1
        assert field(n=4097) == -1 and host(n=4097, g=np.ones(3 * 4097, np.int32)) == -1
        assert field(g=None) == -1 and host(g=None) == -1
        for k in ("o", "d", "a", "work", "walk", "nxt", "s"):
            assert field(**{k: None}) == -1, k
        assert field(g=None, n=0) == 0 and field(md=1 << 24) == 0 and host() == 0
        assert L.vxrt_nav_field_host(h, o3, d3, ag, None, 0, 10, None, hn.ctypes.data, None, hs.ctypes.data) == -1
        assert L.vxrt_nav_field_host(h, o3, d3, ag, None, 0, 10, hw.ctypes.data, None, None, hs.ctypes.data) == -1
        assert L.vxrt_nav_field_host(h, o3, d3, ag, None, 0, 10, hw.ctypes.data, hn.ctypes.data, None, None) == -1
        torch.cuda.synchronize()
        # paths
        r = ctx.nav_field((0, 0, 0), (8, 8, 8), [(1, 1, 1)], vx.NavAgent())

        class Desc(C.Structure):
            _fields_ = [("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("agent", C.c_int32 * 4), ("d_next", C.c_void_p)]
        desc = Desc(o3, d3, ag, r.next.data_ptr())
        st = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
        ln, ss = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        paths = lambda d=C.byref(desc), s=st.data_ptr(), n=4, ms=5, l=ln.data_ptr(), t=ss.data_ptr(): \
            L.vxrt_nav_paths(h, d, s, n, ms, None, l, t, None)
        assert paths() == 0 and paths(n=0) == 0 and paths(ms=65535) == 0
        assert paths(ms=65536) == -1 and paths(d=None) == -1 and paths(s=None) == -1 and paths(l=None) == -1 and paths(t=None) == -1
        for bad in [Desc(o3, d3, ag, None), Desc(o3, (C.c_int32 * 3)(0, 8, 8), ag, r.next.data_ptr()),
                    Desc(o3, d3, (C.c_int32 * 4)(0, 2, 1, 3), r.next.data_ptr())]:
            assert paths(d=C.byref(bad)) == -1
        torch.cuda.synchronize()
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert field() == -1 and host() == -1    # streamed world
        ctx.stream_close()
    finally:
        ctx.close()


def test_headless_example_nav_line(vxo, tmp_path):
    """examples/voxelapp_headless kind 5: the printed summary equals the reference's for the camera's cell"""
    from oracle import vxo_edit
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    col = vox[100, :, 120]
    top = int(np.nonzero(col)[0].max()) + 1 if col.any() else 0
    pos = (100.5, top + 0.5, 120.5)
    path = tmp_path / "path.txt"
    path.write_text("%r %r %r 0 0 0\n%r %r %r 0 0 0\n" % (pos + pos))
    o, d = (40, max(top - 30, 0), 60), (128, 60, 128)
    sf = tmp_path / "edits.txt"
    sf.write_text("1 5 0 %d %d %d %d %d %d\n" % (*o, *d))
    out = subprocess.run([exe, str(edge), "0", str(tmp_path / "nv"), "64", "48", "1", str(path), "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    goal = [tuple(int(np.floor(v)) for v in pos)]
    want = _want(vox, o, d, (1, 2, 1, 3), goal)
    s = want["summary"]
    assert s[1] == 1 and s[3] > 1
    line = [x for x in out.stdout.splitlines() if x.startswith("nav frame")]
    assert line == ["nav frame 1 nodes %d reached %d levels %d max_dist %d" % (s[0], s[3], s[5], s[4])], out.stdout
