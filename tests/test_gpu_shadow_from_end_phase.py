"""Shadow rays launched from the end-of-walk phase of the persistent render kernel (voxelengine_amd/csrc/vxrt_persist2.hpp:
shadow_from_end, the continuation hook of WaveTracerT::phase_end_deferred).

A primary ray that ends on a voxel goes on as its pixel's shadow ray inside the end-of-walk phase -- without parking for the
ray-finished phase -- when the launch is a shaded one with shadows (mode 0), writes no hit-index AOV for any of its views,
its light has no component that is zero or below 2^-40, the kernel is not the multi-view second-bounce instantiation, and the
shadow ray's start lies inside the coarse grid without a -0.0 component.  Every other primary hit takes the ray-finished
phase as before.  Either way the pixel is the same function of its inputs, so every case here compares, byte for byte, the
product kernel (variant 7: its timed and its probe-counting instantiation), the straightforward kernel (variant 1) and the
CPU oracle: frame buffers, hit indices where requested, the four ray counters, and the probe counters of the counting
launches.  FrameStats.dbg[12] of a counting launch of variant 7 is the number of shadow rays that took the new path; each
case says what it must be."""
import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

W, H = 64, 48
INV = helpers.INV
DBG_END_SHADOW = 12


@pytest.fixture(scope="module")
def gpu():
    import torch
    import voxelengine_amd as vx
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ctx = helpers.new_ctx(vx)
    yield vx, ctx, torch
    ctx.close()


def _interior_voxels():
    """64^3: a bumpy floor, two towers and a floating slab (shadow casters), all at least 8 voxels from every face"""
    rng = np.random.default_rng(3)
    v = np.zeros((64, 64, 64), bool)
    h = rng.integers(2, 9, size=(48, 48))
    for y in range(8):
        v[8:56, 8 + y, 8:56] = h > y
    v[20:24, 8:40, 20:24] = True
    v[40:44, 8:30, 30:36] = True
    v[28:44, 34:36, 36:48] = True
    return v


def _edge_voxels():
    """64^3: a low floor, solid voxels in the top layer over half of the world and walls along the +x and +z faces: hits on
    their outer faces put the shadow ray's start outside the grid with the light (1,1,1)/sqrt(3)"""
    v = np.zeros((64, 64, 64), bool)
    v[:, 0:3, :] = True
    v[24:64, 63, 0:40] = True
    v[63, :, :] = True
    v[:, :, 63] = True
    v[10:20, 3:20, 10:20] = True
    return v


def _solid_block_voxels():
    v = np.zeros((64, 64, 64), bool)
    v[:, 0:2, :] = True
    v[24:40, 24:40, 24:40] = True  # the cameras of the hit-at-entry case sit inside and beside this block
    v[8:16, 2:12, 40:48] = True
    return v


@pytest.fixture(scope="module")
def worlds(vxo):
    return {"interior": vxo.World.from_voxels(_interior_voxels(), 8), "edge": vxo.World.from_voxels(_edge_voxels(), 8),
            "block": vxo.World.from_voxels(_solid_block_voxels(), 8)}


def _cam(vxo, pos, target):
    """a camera at `pos` that looks at `target`: (origin, fwd, up, right), an orthonormal frame in binary32"""
    f = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, (0.0, 1.0, 0.0))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    as32 = lambda v: tuple(float(np.float32(c)) for c in v)
    return (as32(pos), as32(f), as32(u), as32(r))


INTERIOR_CAMS = [((32.0, 50.0, 32.0), (32.0, 10.0, 30.0)), ((12.5, 45.0, 50.25), (32.0, 12.0, 32.0)),
                 ((52.0, 40.0, 12.0), (30.0, 10.0, 34.0)), ((30.0, 48.0, 10.0), (32.0, 10.0, 40.0))]


def _oracle(vxo, w, cams, okw, frame_numbers, light, want_hit, width=W, height=H, **render_kw):
    """the oracle's frames of `cams`: [(fb, hit indices)], and the sums of its ray and probe counters"""
    ckw = dict(mode=okw.get("mode", 0), checkerboard=int(okw.get("checkerboard", False)), shadow=int(okw.get("shadow", False)),
               bounce_samples=okw.get("bounce_samples", 0), bounce_all_hits=int(okw.get("bounce_all_hits", False)),
               ortho=int(okw.get("ortho", False)), bounce_depth=okw.get("bounce_depth", 1), ortho_size=(60.0, 60.0), light_dir=light)
    frames, rays, probes = [], np.zeros(4, np.int64), np.zeros(3, np.int64)
    for (pos, f, u, r), fn in zip(cams, frame_numbers):
        p = vxo.make_params(width, height, pos, f, u, r, frame_number=fn, **ckw)
        out = w.render(p, fb=np.zeros((height, width, 4), np.uint8), want_hit=want_hit, nthreads=16, **render_kw)
        st = out["stats"]
        rays += (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits)
        probes += (st.probes.coarse_probes, st.probes.brick_entries, st.probes.fine_probes)
        frames.append((out["fb"], out["hit"]))
    return frames, rays, probes


def _launch(gpu, cams, okw, frame_numbers, variant, stats, hit_views, multi, width=W, height=H):
    """one launch (multi: RenderViews of all `cams`; else one RenderScreen per camera): frames, hit indices, summed stats"""
    vx, ctx, torch = gpu
    ctx.set_kernel_variant(variant)
    try:
        fbs = [torch.zeros((height, width, 4), dtype=torch.uint8, device="cuda") for _ in cams]
        hits = [torch.full((height, width), -7, dtype=torch.int64, device="cuda") if k in hit_views else None for k in range(len(cams))]
        ctx.frame_stats()
        if multi:
            opts = vx.RenderOptions(collect_stats=stats, **okw)
            assert ctx.kernel_for_launch(width, height, opts, nviews=len(cams)) == (7 if variant == 4 else variant)
            ctx.RenderViews(width, height, [dict(fb=fbs[k], origin=c[0], fwd=c[1], up=c[2], right=c[3], frame_number=frame_numbers[k],
                                                 hit_aov=hits[k]) for k, c in enumerate(cams)], opts)
        else:
            for k, c in enumerate(cams):
                opts = vx.RenderOptions(collect_stats=stats, frame_number=frame_numbers[k], **okw)
                assert ctx.kernel_for_launch(width, height, opts) == (7 if variant == 4 else variant)
                ctx.RenderScreen(width, height, fbs[k], c[0], c[1], c[2], c[3], opts, hit_aov=hits[k])
        st = ctx.frame_stats()
        return [f.cpu().numpy() for f in fbs], [None if h is None else h.cpu().numpy() for h in hits], st
    finally:
        ctx.set_kernel_variant(4)


def _check(gpu, vxo, w, cams, okw, *, multi=False, hit_views=(), light=(INV, INV, INV), frame_numbers=None):
    """All three kernels against the oracle on `cams`; returns (shadow rays launched from the end-of-walk phase, shadow rays,
    primary hits) of variant 7's counting launch."""
    vx, ctx, torch = gpu
    frame_numbers = frame_numbers or [3 + k for k in range(len(cams))]
    ctx.SetEnvironment(light, (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    ctx.SetOrthoWindowSize(60.0, 60.0)
    want, rays, probes = _oracle(vxo, w, cams, okw, frame_numbers, light, bool(hit_views))
    counter = None
    for variant, stats in ((4, False), (4, True), (1, False), (1, True)):
        fbs, hits, st = _launch(gpu, cams, okw, frame_numbers, variant, stats, set(hit_views), multi)
        tag = (variant, stats)
        for k in range(len(cams)):
            assert np.array_equal(fbs[k], want[k][0]), (tag, k)
            if k in hit_views:
                assert np.array_equal(hits[k], want[k][1]), (tag, k)
        assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == tuple(int(v) for v in rays), tag
        if stats:
            assert (st.coarse_probes, st.brick_entries, st.fine_probes) == tuple(int(v) for v in probes), tag
            assert st.guard_stray_loads == 0
        if tag == (4, True):
            counter = int(st.dbg[DBG_END_SHADOW])
        elif variant == 1:
            assert int(st.dbg[DBG_END_SHADOW]) == 0
    return counter, int(rays[1]), int(rays[3])


BENCH = dict(shadow=True, bounce_samples=1)


def _view_cams(vxo, cams):
    return [_cam(vxo, p, e) for p, e in cams]


@pytest.mark.parametrize("multi", [False, True])
def test_interior_scene_takes_the_fast_path_for_every_primary_hit(gpu, vxo, worlds, multi):
    """Terrain well inside the grid, the bench light, shadow + one bounce sample: every primary hit's shadow ray starts inside
    the grid, so every shadow ray is launched from the end-of-walk phase -- one view per launch and four views in one."""
    helpers.upload(gpu[1], worlds["interior"])
    cams = _view_cams(vxo, INTERIOR_CAMS if multi else INTERIOR_CAMS[:2])
    counter, shadow, hits = _check(gpu, vxo, worlds["interior"], cams, BENCH, multi=multi)
    assert shadow == hits > (W * H * len(cams)) // 4
    assert counter == shadow


def test_shadow_start_outside_the_grid_keeps_the_ray_finished_phase(gpu, vxo, worlds):
    """Solid voxels in the top layer and along the +x and +z faces, seen from outside and above: with the light
    (1,1,1)/sqrt(3) a hit on one of their outer faces puts position + light_step outside the grid, and that lane must be left
    to the ray-finished phase (begin_ray_deferred's world-entry test); hits on the floor take the fast path."""
    w = worlds["edge"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, [((75.0, 85.0, 25.0), (35.0, 10.0, 30.0)), ((30.0, 80.0, 85.0), (30.0, 10.0, 35.0))])
    # not vacuous (CPU, oracle): the views' primary rays, rebuilt here from the camera model, hit points whose shadow start
    # leaves the grid and points whose start stays inside
    n_out = n_in = 0
    step = np.float32(INV) * np.float32(0.01)
    for pos, f, u, r in cams:
        k = np.float32(np.tan(np.float32(np.pi / 4)))
        xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
        su, sv = (xs / np.float32(W)) * 2 - 1, (ys / np.float32(H)) * 2 - 1
        d = (np.asarray(f, np.float32)[None, None, :] + (su * k * np.float32(W / H))[..., None] * np.asarray(r, np.float32) +
             (sv * k)[..., None] * np.asarray(u, np.float32)).reshape(-1, 3).astype(np.float32)
        o = np.tile(np.asarray(pos, np.float32), (d.shape[0], 1))
        t = w.trace_batch(o, d)
        s0 = (t["pos"][t["hit"] != 0] + step) / np.float32(8.0)
        inside = ((s0 >= 0) & (s0 < 8)).all(axis=1)
        n_in, n_out = n_in + int(inside.sum()), n_out + int((~inside).sum())
    assert n_in > 100 and n_out > 100
    for multi in (False, True):
        counter, shadow, hits = _check(gpu, vxo, w, cams, BENCH, multi=multi)
        assert shadow == hits and 0 < counter < shadow


def test_hit_at_entry(gpu, vxo, worlds):
    """Cameras inside a solid block and a fraction of a voxel outside it: primary rays that hit with no step at all (`at_entry`
    in result(): the position is the ray's start, the normal the world-entry code) and after a step or two; their shadow rays
    start inside solid voxels too."""
    w = worlds["block"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, [((32.3, 32.6, 32.4), (40.0, 30.0, 45.0)), ((40.2, 33.5, 32.5), (30.0, 33.0, 32.0)),
                            ((32.5, 40.1, 32.5), (32.0, 30.0, 33.0)), ((24.5, 24.5, 24.5), (10.0, 5.0, 12.0))])
    inside = cams[:1]
    want = _oracle(vxo, w, inside, BENCH, [3], (INV, INV, INV), False)[1]
    assert want[3] == W * H  # every primary ray of the camera inside the block hits
    for multi in (False, True):
        counter, shadow, hits = _check(gpu, vxo, w, cams, BENCH, multi=multi)
        assert counter == shadow == hits > W * H


def test_hit_index_aov_switches_the_fast_path_off(gpu, vxo, worlds):
    """The hit index is stored by the ray-finished phase's primary branch: a single-view launch with the AOV, and a multi-view
    launch in which ANY view has it (RenderArgs::want_hit_aov), take that branch for every primary hit (counter 0).  Frames do
    not depend on the AOV, and the indices equal the oracle's."""
    w = worlds["interior"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, INTERIOR_CAMS)
    plain, shadow, _ = _check(gpu, vxo, w, cams, BENCH)  # (the frames are compared with the same oracle frames in all four)
    assert plain == shadow > 0
    assert _check(gpu, vxo, w, cams, BENCH, hit_views=(0, 1, 2, 3))[0] == 0
    assert _check(gpu, vxo, w, cams, BENCH, multi=True, hit_views=(1, 3))[0] == 0
    assert _check(gpu, vxo, w, cams, BENCH, multi=True)[0] == shadow
    # one view per launch, the AOV for two of them: the launches without it take the fast path
    got, shadow_all, _ = _check(gpu, vxo, w, cams, BENCH, hit_views=(1, 3))
    assert 0 < got < shadow_all
    assert got == _check(gpu, vxo, w, [cams[0], cams[2]], BENCH, frame_numbers=[3, 5])[0]


@pytest.mark.parametrize("name,okw,expect", [
    ("no shadow", dict(shadow=False, bounce_samples=1), "zero"),
    ("debug view", dict(mode=1, shadow=True, bounce_samples=1), "zero"),
    ("no bounce samples", dict(shadow=True, bounce_samples=0), "all"),
    ("all-hits gate, two samples", dict(shadow=True, bounce_samples=2, bounce_all_hits=True), "all"),
    ("second bounce", dict(shadow=True, bounce_samples=2, bounce_depth=2, bounce_all_hits=True), "all single, zero multi"),
    ("checkerboard", dict(shadow=True, bounce_samples=1, checkerboard=True), "all"),
    ("orthographic", dict(shadow=True, bounce_samples=1, ortho=True), "all"),
])
def test_other_paths(gpu, vxo, worlds, name, okw, expect):
    """What the fast path must leave alone, and what it serves: without shadows and in the debug view no ray follows a primary
    hit from this phase (0); every other option keeps it (all shadow rays) -- except the multi-view second-bounce
    instantiation, which is compiled without the continuation (0)."""
    w = worlds["interior"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, INTERIOR_CAMS[:3])
    for multi in (False, True):
        counter, shadow, hits = _check(gpu, vxo, w, cams, okw, multi=multi)
        assert hits > 0
        if expect == "zero" or (expect == "all single, zero multi" and multi):
            assert counter == 0
        else:
            assert counter == shadow == hits


@pytest.mark.parametrize("count", [2, 3])
def test_strip_shards_reassemble(gpu, vxo, worlds, count):
    """Strip sharding with compact shard buffers: the shards of variant 7 (timed and counting) and variant 1 reassemble to the
    oracle's frame, and their ray counters -- the new one included -- add up to the whole frame's."""
    vx, ctx, torch = gpu
    w = worlds["interior"]
    helpers.upload(ctx, w)
    ctx.SetEnvironment((INV, INV, INV), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    cam = _view_cams(vxo, INTERIOR_CAMS[:1])
    want, rays, probes = _oracle(vxo, w, cam, BENCH, [3], (INV, INV, INV), False)
    pos, f, u, r = cam[0]
    rows = 8
    max_rows = max(vx.compact_rows(H, rows, count, i) for i in range(count))
    stride = max_rows * W * 4
    for variant, stats in ((4, False), (4, True), (1, False)):
        ctx.set_kernel_variant(variant)
        try:
            shards = torch.zeros((count, stride), dtype=torch.uint8, device="cuda")
            ctx.frame_stats()
            for i in range(count):
                ctx.RenderScreen(W, H, shards[i], pos, f, u, r, vx.RenderOptions(strip_rows=rows, strip_count=count, strip_index=i, compact=True,
                                                                                 frame_number=3, collect_stats=stats, **BENCH))
            st = ctx.frame_stats()
            out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            ctx.deinterleave_strips(W, H, rows, count, shards, stride, out)
            assert np.array_equal(out.cpu().numpy(), want[0][0]), (variant, stats)
            assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == tuple(int(v) for v in rays)
            if stats:
                assert (st.coarse_probes, st.brick_entries, st.fine_probes) == tuple(int(v) for v in probes)
                assert int(st.dbg[DBG_END_SHADOW]) == int(rays[1]) > 0
        finally:
            ctx.set_kernel_variant(4)


def test_temporal_accumulation(gpu, vxo, worlds):
    """Temporal accumulation (single-view launches): frames and histories of four frames with a reset equal the oracle's,
    through the fast path (the shaded colour reaches the history in the ray-finished phase as before)."""
    vx, ctx, torch = gpu
    w = worlds["interior"]
    helpers.upload(ctx, w)
    ctx.SetEnvironment((INV, INV, INV), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    pos, f, u, r = _view_cams(vxo, INTERIOR_CAMS[:1])[0]
    for variant, stats in ((4, False), (4, True), (1, False)):
        ctx.set_kernel_variant(variant)
        try:
            acc_c, fb_c = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.uint8)
            acc_g = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            fb_g = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            for frame in range(1, 5):
                reset = frame == 3
                p = vxo.make_params(W, H, pos, f, u, r, frame_number=frame, shadow=1, bounce_samples=1)
                cst = w.render(p, fb=fb_c, accum=acc_c, accum_reset=reset)["stats"]
                ctx.frame_stats()
                ctx.RenderScreen(W, H, fb_g, pos, f, u, r, vx.RenderOptions(frame_number=frame, collect_stats=stats, **BENCH), accum=acc_g,
                                 accum_reset=reset)
                st = ctx.frame_stats()
                assert np.array_equal(fb_g.cpu().numpy(), fb_c), (variant, stats, frame)
                assert np.array_equal(acc_g.cpu().numpy().view(np.uint32), acc_c.view(np.uint32)), (variant, stats, frame)
                assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == (
                    cst.primary_rays, cst.shadow_rays, cst.bounce_rays, cst.primary_hits)
                if stats:
                    assert int(st.dbg[DBG_END_SHADOW]) == cst.shadow_rays > 0
        finally:
            ctx.set_kernel_variant(4)


@pytest.mark.parametrize("light", [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.6, 1e-13, 0.8), (-0.5, 0.7, -0.5)])
def test_special_lights(gpu, vxo, worlds, light):
    """Axis-aligned lights and a light with one component below 2^-40 make every shadow ray `special` (quotients by the
    division, every step validated): such a launch keeps the ray-finished phase's path (counter 0).  A light that shines
    down two axes is an ordinary direction and takes the fast path.  Frames equal the oracle's in every case."""
    w = worlds["interior"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, INTERIOR_CAMS[:2])
    special = min(abs(c) for c in light) < 2.0 ** -40
    for multi in (False, True):
        counter, shadow, hits = _check(gpu, vxo, w, cams, BENCH, multi=multi, light=light)
        assert shadow == hits > 0
        assert counter == (0 if special else shadow)


def test_wide_grid(gpu, vxo):
    """A coarse grid beyond the tracer's packed step counters (1024 cells along x, 8 x 8 across): the wide-grid instantiations
    of the kernel, whose start_walk also arms the CF_OFF_* words for the walks the fast path records."""
    rng = np.random.default_rng(1024)
    X = 1024 * 8
    v = np.zeros((X, 64, 64), bool)
    n_vox = int(X * 64 * 64 * 0.00003)
    v[rng.integers(0, X, n_vox), rng.integers(0, 64, n_vox), rng.integers(0, 64, n_vox)] = True
    v[:, 0, :] = True
    w = vxo.World.from_voxels(v, 8)
    assert w.cdims[0] == 1024
    helpers.upload(gpu[1], w)
    cams = [helpers.camera("A", w.dims, vxo), _cam(vxo, (4000.0, 40.0, 30.0), (4100.0, 0.0, 32.0))]
    for multi in (False, True):
        counter, shadow, hits = _check(gpu, vxo, w, cams, BENCH, multi=multi)
        assert shadow == hits > 0
        # (only a hit on a voxel of the top layer or of a far face -- 3 layers of 64 hold sparse voxels -- starts outside the grid)
        assert shadow // 2 < counter <= shadow
