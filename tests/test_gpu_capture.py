"""Stream capture of render, batch and query launches (include/vxrt.h, "Stream capture"): every call the contract allows is
captured into a graph with torch.cuda.graph in its default (global, strictest) error mode, on ONE side stream, and the
graph's replays are compared with the same references as the eager paths -- frames and batches with the CPU oracle bit for
bit (the colour AOV within COLOR_TOL), queries with tests/ref_*.py and oracle/ref_region.py.  A replay must own what it reads
(the views of a multi-view launch), must be repeatable after the context's rings have wrapped, must see in-capacity edits
of the world, and the calls the contract refuses must leave the capture valid and the context's counters where they were."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_edit, ref_region, vxo_edit
from tests import helpers
from tests import ref_collide, ref_dist, ref_islands, ref_light, ref_lod, ref_surface
from tests.helpers import gen_dense, new_ctx, upload

pytestmark = pytest.mark.gpu

COLOR_TOL = 1e-4
BIG, SMALL = (200, 120), (72, 40)
SHADED = dict(shadow=1, bounce_samples=1)


class Scene:
    def __init__(self, name, ctx, w):
        self.name, self.ctx, self.w = name, ctx, w


@pytest.fixture(scope="module")
def eng():
    import torch
    import voxelengine_amd as vx
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return vx, torch


@pytest.fixture(scope="module")
def side(eng):
    """the one stream everything here is captured on, replayed on and launched on"""
    return eng[1].cuda.Stream()


@pytest.fixture(scope="module")
def worlds(vxo):
    """terrain 256^3 at brick edge 32 (plain shaded frames run the instantiation of their own) and terrain 128^3 at brick
    edge 16 (the general instantiation)"""
    return {"t256": vxo.World.generate(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32),
            "t128": vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16)}


@pytest.fixture(scope="module")
def scenes(eng, worlds):
    vx, _ = eng
    out = {}
    for name, w in worlds.items():
        ctx = new_ctx(vx)
        upload(ctx, w)
        out[name] = Scene(name, ctx, w)
    yield out
    for s in out.values():
        s.ctx.close()


def _stale(H, W):
    return np.random.default_rng(7).integers(0, 255, size=(H, W, 4), dtype=np.uint8)


_ORACLE = {}


def _cam(vxo, cam, dims):
    return helpers.camera(cam, dims, vxo) if isinstance(cam, str) else cam


def _oracle(vxo, name, w, W, H, cam, zero_fb=False, **kw):
    """the oracle's frame (fb over the stale pattern -- or over zeros --, colour and hit AOVs, counters), rendered once per
    case and shared; nobody writes to it"""
    key = (name, W, H, repr(cam), zero_fb, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        pos, f, u, r = _cam(vxo, cam, w.dims)
        p = vxo.make_params(W, H, pos, f, u, r, **kw)
        fb0 = np.zeros((H, W, 4), np.uint8) if zero_fb else _stale(H, W)
        _ORACLE[key] = w.render(p, fb=fb0, want_color=True, want_hit=True, nthreads=16)
    return _ORACLE[key]


def _opts(vx, kw, **extra):
    return vx.RenderOptions(mode=kw.get("mode", 0), checkerboard=bool(kw.get("checkerboard", 0)), shadow=bool(kw.get("shadow", 0)),
                            bounce_samples=kw.get("bounce_samples", 0), ortho=bool(kw.get("ortho", 0)),
                            frame_number=kw.get("frame_number", 1), **extra)


def _view(vxo, w, cam, fb, frame_number):
    pos, f, u, r = _cam(vxo, cam, w.dims)
    return dict(fb=fb, origin=pos, fwd=f, up=u, right=r, frame_number=frame_number)


def _assert_frame(want, fb, col=None, hit=None, tag=None):
    assert np.array_equal(fb.cpu().numpy().reshape(want["fb"].shape), want["fb"]), tag
    if hit is not None:
        assert np.array_equal(hit.cpu().numpy(), want["hit"]), tag
    if col is not None:  # NaN and +-inf exactly where the oracle has them, the finite entries within COLOR_TOL
        got, ref = col.cpu().numpy(), want["color"]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
        assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), tag
        fin = np.isfinite(ref)
        assert np.max(np.abs(got[fin] - ref[fin]), initial=0.0) <= COLOR_TOL, tag


def _capture(torch, side, issue):
    """`issue()` captured on `side` in torch's default capture mode: one stream, no fork or join"""
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        issue()
    return g


def _warm_views(vx, vxo, torch, scene, side):
    """the eager multi-view launch that allocates the context's view slots (the warm-up rule of the capture contract)"""
    with torch.cuda.stream(side):
        tiny = torch.zeros((2, 8, 16, 4), dtype=torch.uint8, device="cuda")
        scene.ctx.RenderViews(16, 8, [_view(vxo, scene.w, c, tiny[j], 1) for j, c in enumerate("AB")], vx.RenderOptions())
    side.synchronize()


# ---- 1. single view ------------------------------------------------------------------------------------------------------
SINGLE = {  # oracle keywords, the AOVs the case asks for
    "plain": (dict(frame_number=2), ()),
    "shadow_bounce": (dict(frame_number=3, **SHADED), ("col", "hit")),
    "checkerboard": (dict(frame_number=5, checkerboard=1, **SHADED), ("hit",)),
    "ortho": (dict(frame_number=4, ortho=1, ortho_size=(60.0, 60.0), shadow=1), ("col",)),
    "debug": (dict(frame_number=6, mode=1), ("col", "hit")),
}


@pytest.mark.parametrize("variant", [4, 1])
@pytest.mark.parametrize("case", list(SINGLE))
def test_single_view_replays_equal_the_oracle(eng, vxo, scenes, side, case, variant):
    """one RenderScreen with an explicit frame number, captured once and replayed three times over a stale framebuffer: each
    replay is the oracle's frame, AOVs included, and stale bytes survive where the oracle leaves them (the checkerboard's
    other half)"""
    vx, torch = eng
    kw, aovs = SINGLE[case]
    for name, (W, H), cam in (("t256", BIG, "A"), ("t128", SMALL, "D")):
        s = scenes[name]
        ctx = s.ctx
        want = _oracle(vxo, name, s.w, W, H, cam, **kw)
        pos, f, u, r = helpers.camera(cam, s.w.dims, vxo)
        stale = torch.from_numpy(_stale(H, W)).cuda()
        fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") if "col" in aovs else None
        hit = torch.full((H, W), -1, dtype=torch.int64, device="cuda") if "hit" in aovs else None
        ctx.SetOrthoWindowSize(*kw.get("ortho_size", (10.0, 10.0)))
        ctx.set_kernel_variant(variant)
        try:
            opts = _opts(vx, kw)
            assert ctx.kernel_for_launch(W, H, opts) == (7 if variant == 4 else 1)
            if case == "plain" and variant == 4:  # the two instantiations of the persistent kernel
                assert ctx.render_specialisation(W, H, opts) == (1 if name == "t256" else 0)
            g = _capture(torch, side, lambda: ctx.RenderScreen(W, H, fb, pos, f, u, r, opts, color_aov=col, hit_aov=hit))
        finally:
            ctx.set_kernel_variant(4)
        assert not fb.any()  # capturing ran nothing
        # the launch's arguments were baked at capture: what the context is told afterwards reaches later launches only
        ctx.SetEnvironment((0.0, 1.0, 0.0), (1, 0, 0), (0, 0, 0))
        ctx.SetFOV(45.0)
        ctx.SetOrthoWindowSize(3.0, 5.0)
        try:
            with torch.cuda.stream(side):
                for k in range(3):
                    fb.copy_(stale)
                    if col is not None:
                        col.zero_()
                    if hit is not None:
                        hit.fill_(-1)
                    g.replay()
                    side.synchronize()
                    _assert_frame(want, fb, col, hit, (case, variant, name, k))
        finally:
            ctx.SetEnvironment((helpers.INV, helpers.INV, helpers.INV), (2, 2, 2), (0.5, 0.5, 0.5))
            ctx.SetFOV(90.0)
            ctx.SetOrthoWindowSize(10.0, 10.0)
        if kw.get("checkerboard"):
            assert (want["fb"] == _stale(H, W)).all(axis=2).sum() >= W * H // 2 - W  # half the frame is stale bytes


# ---- 2. multi view -------------------------------------------------------------------------------------------------------
def _other_cams(vx, dims, n):
    """cameras that are none of helpers.CAMERAS"""
    out = []
    for k in range(n):
        f, u, r = vx.GetDirections((-0.3 - 0.1 * k, 2.1 + 0.7 * k, 0.0))
        out.append(((0.3 * dims[0] + 5.0 * k, 0.95 * dims[1], 0.6 * dims[2]), f, u, r))
    return out


@pytest.mark.parametrize("name,size,nviews", [("t256", BIG, 3), ("t128", SMALL, 16)])
def test_multi_view_graphs_own_their_views(eng, vxo, scenes, side, name, size, nviews):
    """two captured multi-view launches and an eager one, each with its own cameras, frame numbers and buffers: whatever the
    order of the replays, a graph renders the views it was captured with into its own buffers and touches nothing else.  (A
    graph that read its views from memory the capturing call had only borrowed would render the cameras of a later call.)"""
    vx, torch = eng
    s = scenes[name]
    ctx, w = s.ctx, s.w
    W, H = size
    opts = _opts(vx, SHADED)
    _warm_views(vx, vxo, torch, s, side)
    cams = {"a": ("ABC" * 6)[:nviews], "b": ("DAB" * 6)[:nviews]}
    first = {"a": 1, "b": 40}
    bufs = {k: torch.zeros((nviews, H, W, 4), dtype=torch.uint8, device="cuda") for k in cams}
    graphs = {}
    for k in ("a", "b"):
        views = [_view(vxo, w, c, bufs[k][j], first[k] + j) for j, c in enumerate(cams[k])]
        graphs[k] = _capture(torch, side, lambda: ctx.RenderViews(W, H, views, opts))
        del views  # the graph must not need the caller's arrays
    stale = torch.from_numpy(_stale(H, W)).cuda()
    with torch.cuda.stream(side):
        scratch = torch.zeros((4, H, W, 4), dtype=torch.uint8, device="cuda")
        ctx.RenderViews(W, H, [_view(vxo, w, c, scratch[j], 90 + j) for j, c in enumerate(_other_cams(vx, w.dims, 4))], opts)
        for k in ("a", "b", "a"):
            other = "b" if k == "a" else "a"
            for b in bufs.values():
                b.copy_(stale.expand_as(b))
            graphs[k].replay()
            side.synchronize()
            for j, c in enumerate(cams[k]):
                _assert_frame(_oracle(vxo, name, w, W, H, c, frame_number=first[k] + j, **SHADED), bufs[k][j], tag=(k, j))
            assert torch.equal(bufs[other], stale.expand_as(bufs[other])), k


# ---- 3. replay after the rings wrap ----------------------------------------------------------------------------------------
def test_replay_after_the_rings_wrap(eng, vxo, scenes, side):
    """65 eager single-view and 17 eager multi-view launches between capture and replay take every queue head and every view
    slot of the context once more, the graphs' own included: the graphs still render their frames, because the reset of the
    queue head and the stores of the views are nodes of the graph, ordered on the stream with everything else"""
    vx, torch = eng
    s = scenes["t128"]
    ctx, w = s.ctx, s.w
    W, H = SMALL
    opts = _opts(vx, SHADED)
    _warm_views(vx, vxo, torch, s, side)
    fb1 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    fbm = torch.zeros((3, H, W, 4), dtype=torch.uint8, device="cuda")
    pos, f, u, r = helpers.camera("A", w.dims, vxo)
    g1 = _capture(torch, side, lambda: ctx.RenderScreen(W, H, fb1, pos, f, u, r, _opts(vx, dict(frame_number=5, **SHADED))))
    gm = _capture(torch, side, lambda: ctx.RenderViews(W, H, [_view(vxo, w, c, fbm[j], 6 + j) for j, c in enumerate("BCD")], opts))
    stale = torch.from_numpy(_stale(H, W)).cuda()
    with torch.cuda.stream(side):
        tiny = torch.zeros((2, 8, 16, 4), dtype=torch.uint8, device="cuda")
        for _ in range(65):
            ctx.RenderScreen(16, 8, tiny[0], pos, f, u, r, _opts(vx, dict(frame_number=1)))
        for _ in range(17):
            ctx.RenderViews(16, 8, [_view(vxo, w, c, tiny[j], 1) for j, c in enumerate("CD")], vx.RenderOptions())
        fb1.copy_(stale)
        fbm.copy_(stale.expand_as(fbm))
        g1.replay()
        gm.replay()
        side.synchronize()
    _assert_frame(_oracle(vxo, "t128", w, W, H, "A", frame_number=5, **SHADED), fb1, tag="single")
    for j, c in enumerate("BCD"):
        _assert_frame(_oracle(vxo, "t128", w, W, H, c, frame_number=6 + j, **SHADED), fbm[j], tag=("multi", j))


# ---- 4. batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,n", [("one ray per lane", 30000), ("persistent queue", 262145)])
def test_batch_replays_equal_the_oracle(eng, vxo, worlds, side, kernel, n):
    """trace_batch_device with hit and voxel outputs, captured and replayed twice into poisoned outputs: the oracle's batch,
    rays that are no rays included (helpers.mixed_rays).  The queue kernel's ticket counter is reset by a node of the graph;
    n = 262145 leaves a ragged last ticket (as tests/test_gpu_parity.py: one persistent wave per CU makes it the queue's)."""
    vx, torch = eng
    w = worlds["t128"]
    ctx = vx.Context(0)
    try:
        if kernel == "persistent queue":
            ctx.set_persistent_waves_per_cu(1)
        upload(ctx, w)
        o, d = helpers.mixed_rays(w.dims, n, 5)
        cpu = w.trace_batch(o, d, nthreads=16)
        assert 0 < int(cpu["hit"].sum()) < n
        d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        pos = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        steps = torch.empty(n, dtype=torch.int32, device="cuda")
        hit = torch.empty(n, dtype=torch.uint8, device="cuda")
        vox = torch.empty(n, dtype=torch.int64, device="cuda")
        g = _capture(torch, side, lambda: ctx.trace_batch_device(d_o, d_d, n, pos, nrm, steps, hit, vox))
        with torch.cuda.stream(side):
            for k in range(2):
                pos.fill_(-7.0)
                nrm.fill_(-7.0)
                steps.fill_(-7)
                hit.fill_(9)
                vox.fill_(-7)
                g.replay()
                side.synchronize()
                assert np.array_equal(hit.cpu().numpy(), cpu["hit"]), k
                assert np.array_equal(steps.cpu().numpy(), cpu["steps"]), k
                assert np.array_equal(vox.cpu().numpy(), cpu["voxel"]), k
                assert np.array_equal(helpers.float_bits(pos.cpu().numpy()), helpers.float_bits(cpu["pos"])), k
                assert np.array_equal(nrm.cpu().numpy(), cpu["normal"]), k
    finally:
        ctx.close()


# ---- 5. counters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [4, 1])
def test_counters_grow_once_per_replay(eng, vxo, scenes, side, variant):
    """a collect_stats frame in a graph: capturing counts nothing, every replay adds the oracle's ray and probe counts"""
    vx, torch = eng
    s = scenes["t256"]
    ctx, w = s.ctx, s.w
    W, H = BIG
    kw = dict(frame_number=3, **SHADED)
    want = _oracle(vxo, "t256", w, W, H, "A", **kw)
    pos, f, u, r = helpers.camera("A", w.dims, vxo)
    fb = torch.from_numpy(_stale(H, W)).cuda()
    ctx.set_kernel_variant(variant)
    try:
        ctx.frame_stats()
        g = _capture(torch, side, lambda: ctx.RenderScreen(W, H, fb, pos, f, u, r, _opts(vx, kw, collect_stats=True)))
    finally:
        ctx.set_kernel_variant(4)
    assert ctx.frame_stats().total_rays() == 0
    with torch.cuda.stream(side):
        for _ in range(3):
            g.replay()
    st, cst = ctx.frame_stats(), want["stats"]   # (synchronises the device)
    _assert_frame(want, fb)
    assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == (
        3 * cst.primary_rays, 3 * cst.shadow_rays, 3 * cst.bounce_rays, 3 * cst.primary_hits)
    assert (st.coarse_probes, st.brick_entries, st.fine_probes) == (
        3 * cst.probes.coarse_probes, 3 * cst.probes.brick_entries, 3 * cst.probes.fine_probes)
    assert cst.primary_rays == W * H and cst.shadow_rays > 0 and cst.bounce_rays > 0


# ---- 6. deinterleave -----------------------------------------------------------------------------------------------------
def test_strip_shards_and_deinterleave_in_one_graph(eng, vxo, scenes, side):
    """two compact strip shards (16-row strips; the last strip of a 120-row frame is ragged) rendered into one shard buffer and
    scattered by vxrt_deinterleave_strips, all in one graph; and the same for the two views of a multi-view step with
    vxrt_deinterleave_views: the replayed full frames are the oracle's"""
    vx, torch = eng
    s = scenes["t256"]
    ctx, w = s.ctx, s.w
    W, H = BIG
    rows, count = 16, 2
    shard_bytes = max(vx.compact_rows(H, rows, count, i) for i in range(count)) * W * 4
    strip = lambda i, **kw: _opts(vx, kw, strip_rows=rows, strip_count=count, strip_index=i, compact=True)
    kw = dict(frame_number=2, **SHADED)
    pos, f, u, r = helpers.camera("A", w.dims, vxo)
    shards = torch.zeros((count, shard_bytes), dtype=torch.uint8, device="cuda")
    full = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")

    def one_view():
        for i in range(count):
            ctx.RenderScreen(W, H, shards[i], pos, f, u, r, strip(i, **kw))
        ctx.deinterleave_strips(W, H, rows, count, shards, shard_bytes, full)

    g = _capture(torch, side, one_view)
    with torch.cuda.stream(side):
        shards.zero_()
        full.fill_(9)
        g.replay()
        side.synchronize()
    _assert_frame(_oracle(vxo, "t256", w, W, H, "A", zero_fb=True, **kw), full, tag="strips")

    _warm_views(vx, vxo, torch, s, side)
    nv, step_bytes = 2, 2 * shard_bytes
    shards2 = torch.zeros((count, step_bytes), dtype=torch.uint8, device="cuda")
    full2 = torch.zeros((nv, H, W, 4), dtype=torch.uint8, device="cuda")

    def two_views():
        for i in range(count):
            at = shards2.data_ptr() + i * step_bytes
            ctx.RenderViews(W, H, [_view(vxo, w, c, at + j * shard_bytes, 7 + j) for j, c in enumerate("AD")], strip(i, **SHADED))
        ctx.deinterleave_views(W, H, rows, count, shards2, step_bytes, shard_bytes, nv, full2, W * H * 4)

    g2 = _capture(torch, side, two_views)
    with torch.cuda.stream(side):
        shards2.zero_()
        full2.fill_(9)
        g2.replay()
        side.synchronize()
    for j, c in enumerate("AD"):
        _assert_frame(_oracle(vxo, "t256", w, W, H, c, zero_fb=True, frame_number=7 + j, **SHADED), full2[j], tag=("views", j))


# ---- 7. queries ----------------------------------------------------------------------------------------------------------
def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _grid(t, dims, dtype):
    return t.cpu().numpy().view(dtype).reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)


def test_queries_in_one_graph_follow_in_capacity_edits(eng, vxo, side):
    """the eight stream-ordered queries and a render captured in ONE graph on a box that overhangs the world on two faces: a
    replay gives every reference on the world as it is; after an edit batch and a stamp that create and free bricks inside
    the reserved pool, a replay of the SAME graph gives every reference on the edited world"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    X = 128
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, X, X), X, X, X)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        ctx.edit_reserve((X // 16) ** 3)  # a brick for every cell: no edit can grow the pool
        capacity = ctx.edit_voxels([]).pool_capacity
        assert capacity >= (X // 16) ** 3
        L, h, dev = ctx._L, ctx._h, "cuda"
        heights = np.where(vox.any(1), X - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
        top = int(np.median(heights[:40, 96:]))
        o, d = (-5, top - 12, 100), (40, 24, 37)  # x from -5, z to 136: over the world's x-lo and z-hi faces
        nvox, nwords = d[0] * d[1] * d[2], vx.region_words(d)
        i3 = lambda v: (C.c_int32 * 3)(*v)
        tensor = lambda n, dt: torch.zeros(max(int(n), 1), dtype=dt, device=dev)
        work = lambda nbytes: torch.zeros(max(int(nbytes), 4), dtype=torch.uint8, device=dev)
        rng = np.random.default_rng(11)
        bodies = ref_collide.random_bodies(rng, (X, X, X), 256)
        assert len(bodies) == 256
        emitters = [(3, top + 2, 110, 15), (20, top + 6, 120, 9), (-2, top, 130, 12), (30, top - 3, 104, 14), (500, 0, 0, 7)]
        radius, shift, threshold, order, max_islands = 6, 1, 3, (1, 0, 2), 4096
        W, H = SMALL
        kw = dict(frame_number=4, **SHADED)
        cam = helpers.camera("A", (X, X, X), vxo)

        def references(v):
            box = ref_region.read_region(v, o, d)
            surf = ref_surface.extract(v, o, d, ref_surface.CAP)
            return dict(region=vx.pack_region(box), overlap=ref_collide.overlap_boxes(v, bodies), move=ref_collide.move_boxes(v, bodies, order),
                        dist=ref_dist.fast(v, o, d, radius, ref_dist.TO_SOLID), light=ref_light.light_field(v, o, d, emitters),
                        surface=surf, lod=ref_lod.downsample(v, o, d, shift, threshold), islands=ref_islands.fast(box, o),
                        frame=vxo.World.from_voxels(v, 16).render(vxo.make_params(W, H, *cam, **kw), fb=_stale(H, W), nthreads=16))

        rng2 = np.random.default_rng(12)
        ops = [(0, 0, (0, 0, 96), (15, X - 1, X - 1)),                      # frees every brick of two columns of cells
               (0, 1, (3, top + 3, 105), (12, top + 8, 115)),               # a slab in the air above them: an island
               (1, 0, (30, top - 4, 110), (5, 0, 0)), (0, 1, (60, X - 10, 60), (70, X - 3, 70))]  # a hole; bricks in the sky
        stamps = [((18, top - 2, 108), rng2.random((14, 12, 16)) < 0.3, vx.STAMP_UNION)]
        edited = ref_region.apply_stamps(ref_edit.apply_edits(vox, ops), stamps)
        want = [references(vox), references(edited)]
        cap_quads = max(len(r["surface"].quads) for r in want) + 8

        d_bodies = torch.from_numpy(bodies).to(dev)
        d_emit = torch.from_numpy(np.asarray(emitters, np.int32)).to(dev)
        out = dict(
            region=tensor(nwords, torch.int32), counts=tensor(256, torch.int32), cflags=tensor(256, torch.int32),
            lohi=tensor(256 * 6, torch.float32), mflags=tensor(256, torch.int32),
            dist=tensor(nvox, torch.int16), dist_sum=tensor(6, torch.int32),
            light=tensor(nvox, torch.uint8), light_sum=tensor(42, torch.int32),
            quads=tensor(cap_quads * 2, torch.int32), verts=tensor(cap_quads * 12, torch.int32), tris=tensor(cap_quads * 6, torch.int32),
            surf_sum=tensor(16, torch.int32),
            lod=tensor(nwords, torch.int32), lod_counts=tensor(nvox, torch.int16), lod_sum=tensor(8, torch.int32),
            floating=tensor(nwords, torch.int32), labels=tensor(nvox, torch.int32), table=tensor(max_islands * 8, torch.int32),
            isl_sum=tensor(3, torch.int32), fb=torch.zeros((H, W, 4), dtype=torch.uint8, device=dev))
        ws = dict(dist=work(L.vxrt_distance_workspace_bytes(i3(d), radius)), light=work(L.vxrt_light_workspace_bytes(i3(d), 3)),
                  surf=work(L.vxrt_surface_workspace_bytes(i3(d))), lod=work(L.vxrt_lod_workspace_bytes(i3(d), shift)),
                  isl=work(L.vxrt_islands_workspace_bytes(i3(d))))
        assert all(t.numel() > 4 for t in ws.values())
        p = lambda t: t.data_ptr()

        def issue():
            st = side.cuda_stream
            N.check(L.vxrt_read_region(h, i3(o), i3(d), p(out["region"]), st))
            N.check(L.vxrt_overlap_boxes(h, p(d_bodies), 256, p(out["counts"]), p(out["cflags"]), st))
            N.check(L.vxrt_move_boxes(h, p(d_bodies), 256, i3(order), p(out["lohi"]), p(out["mflags"]), st))
            N.check(L.vxrt_distance_field(h, i3(o), i3(d), radius, ref_dist.TO_SOLID, p(ws["dist"]), p(out["dist"]), p(out["dist_sum"]), st))
            N.check(L.vxrt_light_field(h, i3(o), i3(d), p(d_emit), len(emitters), 3, p(ws["light"]), p(out["light"]),
                                       p(out["light_sum"]), st))
            N.check(L.vxrt_extract_surface(h, i3(o), i3(d), ref_surface.CAP, p(ws["surf"]), p(out["quads"]), cap_quads, p(out["verts"]),
                                           p(out["tris"]), p(out["surf_sum"]), st))
            N.check(L.vxrt_downsample_region(h, i3(o), i3(d), shift, threshold, p(ws["lod"]), p(out["lod"]), p(out["lod_counts"]),
                                             p(out["lod_sum"]), st))
            N.check(L.vxrt_find_islands(h, i3(o), i3(d), ref_islands.FACES | ref_islands.FLOOR, p(ws["isl"]), p(out["floating"]),
                                        p(out["labels"]), p(out["table"]), max_islands, p(out["isl_sum"]), st))
            ctx.RenderScreen(W, H, out["fb"], *cam, _opts(vx, kw))

        g = _capture(torch, side, issue)

        def replay_and_check(r, tag):
            with torch.cuda.stream(side):
                for t in out.values():
                    t.fill_(0x5A if t.dtype != torch.float32 else -7.0)
                out["fb"].copy_(torch.from_numpy(_stale(H, W)).to(dev))
                g.replay()
                side.synchronize()
            assert np.array_equal(_u32(out["region"]), r["region"]), tag
            assert np.array_equal(_u32(out["counts"]), r["overlap"][0]) and np.array_equal(_u32(out["cflags"]), r["overlap"][1]), tag
            assert np.array_equal(helpers.float_bits(out["lohi"].cpu().numpy().reshape(-1, 6)), helpers.float_bits(r["move"][0])), tag
            assert np.array_equal(_u32(out["mflags"]), r["move"][1]), tag
            assert np.array_equal(_grid(out["dist"], d, np.uint16), r["dist"]["dist2"]), tag
            s = [int(v) for v in _u32(out["dist_sum"])]
            assert (s[0], s[1], s[2], s[3], s[4] | s[5] << 32) == r["dist"]["summary"], tag
            assert np.array_equal(_grid(out["light"], d, np.uint8), r["light"]["levels"]), tag
            assert ref_light.summary_from_words(_u32(out["light_sum"])) == r["light"]["summary"], tag
            surf = r["surface"]
            n = len(surf.quads)
            assert np.array_equal(_u32(out["surf_sum"]), surf.summary) and n > 0, tag
            assert np.array_equal(_u32(out["quads"]).reshape(-1, 2)[:n], surf.quads), tag
            assert np.array_equal(out["verts"].cpu().numpy().reshape(-1, 3)[:4 * n], surf.vertices), tag
            assert np.array_equal(_u32(out["tris"]).reshape(-1, 3)[:2 * n], surf.triangles), tag
            assert np.array_equal(_u32(out["lod"]), r["lod"].words), tag
            assert np.array_equal(out["lod_counts"].cpu().numpy().view(np.uint16), r["lod"].flat), tag
            assert np.array_equal(_u32(out["lod_sum"]), r["lod"].summary), tag
            isl = r["islands"]
            assert tuple(int(v) for v in _u32(out["isl_sum"])) == isl["summary"], tag
            assert np.array_equal(_u32(out["floating"]), vx.pack_region(isl["floating"])), tag
            assert np.array_equal(_grid(out["labels"], d, np.uint32), isl["labels"]), tag
            rows = out["table"].cpu().numpy().reshape(-1, 8)[:isl["summary"][1]]
            assert np.array_equal(ref_islands.table_rows(rows), isl["table"]), tag
            assert np.array_equal(out["fb"].cpu().numpy(), r["frame"]["fb"]), tag

        replay_and_check(want[0], "as uploaded")
        st1 = ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        st2 = ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        assert st1.bricks_created > 0 and st1.bricks_freed > 0 and st2.bricks_touched > 0
        assert st1.pool_capacity == capacity and st2.pool_capacity == capacity  # nothing moved: the graph's addresses hold
        assert want[1]["islands"]["summary"][1] > want[0]["islands"]["summary"][1]  # the slab in the air
        assert not np.array_equal(want[0]["frame"]["fb"], want[1]["frame"]["fb"])
        replay_and_check(want[1], "edited")
    finally:
        ctx.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_capture_usable(eng, vxo, worlds, side):
    """every call the contract refuses under capture returns VXRT_ERR_INVALID with a message that names capture, enqueues
    nothing and counts nothing: a valid launch issued afterwards in the SAME capture is captured, the capture ends without
    error and replays the oracle's frame, and the context's frame counter is where it was"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    w = worlds["t128"]
    W, H = SMALL
    ctx, fresh = new_ctx(vx), new_ctx(vx)
    try:
        upload(ctx, w)
        upload(fresh, w)
        warm = Scene("t128", ctx, w)
        _warm_views(vx, vxo, torch, warm, side)  # explicit frame numbers: the context's counter stays at 0
        pos, f, u, r = helpers.camera("A", w.dims, vxo)
        fb = torch.zeros((3, H, W, 4), dtype=torch.uint8, device="cuda")
        n = 1000
        o, d = helpers.mixed_rays(w.dims, n, 3)
        d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        pos_o = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        nrm_o = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        steps_o = torch.zeros(n, dtype=torch.int32, device="cuda")
        # a navigation field whose arguments are all valid
        nd, agent = (32, 16, 32), vx.NavAgent()._c()
        i3 = lambda v: (C.c_int32 * 3)(*v)
        nav_work = torch.zeros(int(ctx._L.vxrt_nav_workspace_bytes(i3(nd), C.byref(agent))), dtype=torch.uint8, device="cuda")
        walk = torch.zeros(vx.region_words(nd), dtype=torch.int32, device="cuda")
        nxt = torch.zeros(nd[0] * nd[1] * nd[2], dtype=torch.uint8, device="cuda")
        nav_sum = torch.zeros(8, dtype=torch.int32, device="cuda")
        refused = lambda: pytest.raises(vx.VxrtError, match=r"vxrt error -1: .*capture")
        kw = dict(frame_number=9, **SHADED)
        poison = _stale(H, W)
        fb[:] = torch.from_numpy(poison).cuda()
        nav_work.fill_(0x5A)

        def issue():
            with refused():  # the default frame_number = -1
                ctx.RenderScreen(W, H, fb[0], pos, f, u, r, vx.RenderOptions())
            with refused():  # -1 in one view of several
                ctx.RenderViews(W, H, [_view(vxo, w, "A", fb[0], 1), _view(vxo, w, "B", fb[1], -1), _view(vxo, w, "C", fb[2], 3)],
                                vx.RenderOptions())
            with refused():
                ctx.trace_batch_device(d_o, d_d, n, pos_o, nrm_o, steps_o, want_stats=True)
            with refused():
                N.check(ctx._L.vxrt_nav_field(ctx._h, i3((40, 40, 40)), i3(nd), agent, None, 0, 1 << 24, nav_work.data_ptr(),
                                              walk.data_ptr(), nxt.data_ptr(), None, nav_sum.data_ptr(), side.cuda_stream))
            with refused():  # no view slots yet: the first multi-view launch of a context allocates them
                fresh.RenderViews(W, H, [_view(vxo, w, c, fb[j], 1 + j) for j, c in enumerate("AB")], vx.RenderOptions())
            ctx.RenderScreen(W, H, fb[2], pos, f, u, r, _opts(vx, kw))

        g = _capture(torch, side, issue)
        torch.cuda.synchronize()
        # nothing was enqueued by a refused call, in the capture or outside it
        assert np.array_equal(fb[0].cpu().numpy(), poison) and np.array_equal(fb[1].cpu().numpy(), poison)
        assert not steps_o.any() and not nav_sum.any() and bool((nav_work == 0x5A).all())
        with torch.cuda.stream(side):
            g.replay()
            side.synchronize()
        _assert_frame(_oracle(vxo, "t128", w, W, H, "A", **kw), fb[2], tag="valid launch after the refusals")
        assert np.array_equal(fb[0].cpu().numpy(), poison) and np.array_equal(fb[1].cpu().numpy(), poison)
        assert not steps_o.any() and not nav_sum.any()
        # the frame counter did not move: the first counted frames of both contexts are frames 0, then 1
        cb = dict(checkerboard=1, bounce_samples=1)
        for c in (ctx, fresh):
            for number in (0, 1):
                with torch.cuda.stream(side):
                    fb[0].copy_(torch.from_numpy(poison).cuda())
                    c.RenderScreen(W, H, fb[0], pos, f, u, r, vx.RenderOptions(checkerboard=True, bounce_samples=1))
                    side.synchronize()
                _assert_frame(_oracle(vxo, "t128", w, W, H, "A", frame_number=number, **cb), fb[0], tag=("counter", number))
        # and the refused context renders several views once it is asked outside a capture
        with torch.cuda.stream(side):
            fresh.RenderViews(W, H, [_view(vxo, w, c, fb[j], 1 + j) for j, c in enumerate("AB")], _opts(vx, SHADED))
            side.synchronize()
        for j, c in enumerate("AB"):
            _assert_frame(_oracle(vxo, "t128", w, W, H, c, frame_number=1 + j, **SHADED), fb[j], tag=("fresh", j))
    finally:
        ctx.close()
        fresh.close()
