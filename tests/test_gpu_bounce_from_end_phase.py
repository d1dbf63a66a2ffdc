"""Bounce samples of shadowed pixels launched from the end-of-walk phase of the persistent render kernel
(voxelengine_amd/csrc/vxrt_persist2.hpp: bounce_from_end, the second continuation of WaveTracerT::phase_end_deferred's hook).

A shadow ray that ends on a voxel goes on as its pixel's bounce sample 0 inside the end-of-walk phase -- without parking for the
ray-finished phase -- when the launch is a shaded one with shadows and at least one bounce sample, writes no hit-index AOV, its
light is finite and has no component that is zero or below 2^-40, the kernel is not a second-bounce instantiation, and the
sample ray is on the tracer's fast path from inside the grid (begin_ray_inside_fast: a start inside the coarse grid without a
sign bit, no direction component below 2^-40).  Every other bounce sample is launched by the ray-finished phase as before.
Either way the pixel is the same function of its inputs, so every case compares, byte for byte, the product kernel (variant 7:
timed and counting), the straightforward kernel (variant 1) and the CPU oracle: frames, the four ray counters and the probe
counters.  Context.loop_counters()["end_bounce"] of a counting launch of variant 7 is the number of samples that took the new
path; each case states what it must be, derived on the CPU from the oracle alone (_expected)."""
import math

import numpy as np
import pytest

from tests import helpers
from tests import test_gpu_shadow_from_end_phase as sfe

pytestmark = pytest.mark.gpu

W, H = sfe.W, sfe.H
INV = helpers.INV
f32 = np.float32
BENCH = dict(shadow=True, bounce_samples=1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import voxelengine_amd as vx
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ctx = helpers.new_ctx(vx)
    yield vx, ctx, torch
    ctx.close()


def _common_voxels():
    """256^3 (8 coarse cells an axis at brick edge 32, the smallest grid of that brick edge the world layout allows): a bumpy
    floor, two towers and a floating slab, well inside"""
    rng = np.random.default_rng(9)
    v = np.zeros((256, 256, 256), bool)
    h = rng.integers(2, 17, size=(192, 192))
    for y in range(16):
        v[32:224, 16 + y, 32:224] = h > y
    v[80:92, 16:88, 80:92] = True
    v[160:176, 16:60, 120:140] = True
    v[100:180, 72:76, 140:200] = True
    return v


@pytest.fixture(scope="module")
def worlds(vxo):
    return {"interior": vxo.World.from_voxels(sfe._interior_voxels(), 8), "edge": vxo.World.from_voxels(sfe._edge_voxels(), 8),
            "common": vxo.World.from_voxels(_common_voxels(), 32)}


COMMON_CAMS = [((128.0, 116.0, 128.0), (120.0, 20.0, 132.0)), ((41.0, 100.0, 200.5), (128.0, 24.0, 128.0)),
               ((220.0, 90.0, 48.0), (120.0, 20.0, 140.0)), ((120.0, 110.0, 36.0), (128.0, 20.0, 160.0))]


def _ray_dirs(width, height, fwd, up, right):
    """getRayDirection (Renderer.cu:44-59) at FOV 90 in binary32, one ray per pixel, row-major"""
    t = f32(math.tan(float(f32(90.0 * 3.1415 / 180.0) / f32(2.0))))
    kx, ky = f32(t * (f32(width) / f32(height))), t
    su = (np.arange(width, dtype=f32) / f32(width)) * f32(2) - f32(1)
    sv = (np.arange(height, dtype=f32) / f32(height)) * f32(2) - f32(1)
    su, sv = np.meshgrid(su, sv)
    x, y, z = [(f32(fwd[a]) + (su * kx) * f32(right[a])) + (sv * ky) * f32(up[a]) for a in range(3)]
    inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z, dtype=f32)
    return np.stack([x * inv, y * inv, z * inv], axis=-1).astype(f32).reshape(-1, 3)


_EXPECTED = {}


def _expected(vxo, w, key, cams, frame_numbers, light=(INV, INV, INV), width=W, height=H):
    """(samples the hook must launch, shadowed pixels) of plain frames of `cams`, from the oracle alone: the primary rays are
    rebuilt from the camera model and traced (World.trace_batch; their hit voxels must be the oracle frame's hit indices), the
    shadow rays of the hits are traced, and a shadowed pixel counts when its sample 0 starts inside the coarse grid without a
    sign bit and the oracle's census of a one-sample frame flags neither a special bounce ray nor a sample direction whose
    squared length is not ordinary.  Sample 0 does not depend on the sample count or on the all-hits gate."""
    memo = (key, np.asarray(cams, np.float64).tobytes(), tuple(frame_numbers), tuple(light), width, height)
    if memo in _EXPECTED:
        return _EXPECTED[memo]
    L = np.asarray(light, f32)
    sray = (L * (f32(1.0) / np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2], dtype=f32))).astype(f32)
    step = (sray * f32(0.01)).astype(f32)
    total = shadowed = 0
    for (pos, f, u, r), fn in zip(cams, frame_numbers):
        d = _ray_dirs(width, height, f, u, r)
        t = w.trace_batch(np.tile(np.asarray(pos, f32), (d.shape[0], 1)), d, nthreads=16)
        hit = t["hit"] != 0
        p = vxo.make_params(width, height, pos, f, u, r, frame_number=fn, shadow=1, bounce_samples=1, light_dir=light)
        out = w.render(p, fb=np.zeros((height, width, 4), np.uint8), want_hit=True, want_census=True, nthreads=16)
        assert np.array_equal(out["hit"].reshape(-1), np.where(hit, t["voxel"], -1)), "the rebuilt primary rays are the frame's"
        hp, n = t["pos"][hit], -t["normal"][hit]
        sh = w.trace_batch(hp + step, np.tile(sray, (hp.shape[0], 1)), nthreads=16)["hit"] != 0
        start = ((hp + n * f32(0.01)) / f32(w.factor)).astype(f32)
        inside = ((start.view(np.uint32) >> 31) == 0).all(axis=1) & (start < np.asarray(w.cdims, f32)).all(axis=1)
        cen = out["census"].reshape(-1)[hit]
        plain = (cen & (vxo.CEN_SPECIAL_BOUNCE | vxo.CEN_BOUNCE_DIR | vxo.CEN_INVALID)) == 0
        total += int((sh & inside & plain).sum())
        shadowed += int(sh.sum())
    _EXPECTED[memo] = (total, shadowed)
    return total, shadowed


def _check(gpu, vxo, w, cams, okw, *, multi=False, hit_views=(), light=(INV, INV, INV), frame_numbers=None, common=None):
    """All three kernels against the oracle on `cams` (sfe._oracle / sfe._launch); returns (bounce samples launched from the
    end-of-walk phase by variant 7's counting launch, bounce rays of the frames).  `common`: the instantiation the launches
    must take (render_specialisation)."""
    vx, ctx, torch = gpu
    frame_numbers = frame_numbers or [3 + k for k in range(len(cams))]
    ctx.SetEnvironment(light, (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    ctx.SetOrthoWindowSize(60.0, 60.0)
    if common is not None:
        assert not hit_views
        assert ctx.render_specialisation(W, H, vx.RenderOptions(**okw), nviews=len(cams) if multi else 0) == common
    want, rays, probes = sfe._oracle(vxo, w, cams, okw, frame_numbers, light, bool(hit_views))
    counter = None
    for variant, stats in ((4, False), (4, True), (1, False), (1, True)):
        fbs, hits, st = sfe._launch(gpu, cams, okw, frame_numbers, variant, stats, set(hit_views), multi)
        loop = ctx.loop_counters()
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
            counter = loop["end_bounce"]
        else:
            assert loop["end_bounce"] == 0, tag  # (the timed instantiation and variant 1 count nothing)
    return counter, int(rays[2])


def _view_cams(vxo, cams):
    return [sfe._cam(vxo, p, e) for p, e in cams]


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("world", ["interior", "common"])
def test_shadowed_pixels_launch_their_first_sample_from_the_end_of_walk_phase(gpu, vxo, worlds, world, multi):
    """Terrain well inside the grid, the bench's options: every shadowed pixel's sample 0 starts inside the grid, so all of them
    but the few with a special direction come from the hook.  Brick edge 8 runs the general instantiations, the world of brick
    edge 32 the COMMON ones (asserted)."""
    w = worlds[world]
    helpers.upload(gpu[1], w)
    all_cams = COMMON_CAMS if world == "common" else sfe.INTERIOR_CAMS
    cams = _view_cams(vxo, all_cams if multi else all_cams[:2])
    fns = [3 + k for k in range(len(cams))]
    expect, shadowed = _expected(vxo, w, world, cams, fns)
    assert shadowed > 200 and 0 < expect <= shadowed
    counter, bounce = _check(gpu, vxo, w, cams, BENCH, multi=multi, common=1 if world == "common" else 0)
    assert counter == expect and bounce >= counter


@pytest.mark.parametrize("okw", [dict(shadow=True, bounce_samples=3), dict(shadow=True, bounce_samples=1, bounce_all_hits=True),
                                 dict(shadow=True, bounce_samples=3, bounce_all_hits=True)])
def test_only_sample_zero_of_a_shadowed_pixel_comes_from_the_hook(gpu, vxo, worlds, okw):
    """Three samples, and the all-hits gate (lit pixels bounce too, from the ray-finished phase: their shadow ray missed): the
    hook's count stays the number of shadowed pixels on its fast path."""
    for world, common in (("interior", 0), ("common", 1)):
        w = worlds[world]
        helpers.upload(gpu[1], w)
        cams = _view_cams(vxo, (COMMON_CAMS if common else sfe.INTERIOR_CAMS)[:3])
        expect, _ = _expected(vxo, w, world, cams, [3, 4, 5])
        for multi in (False, True):
            counter, bounce = _check(gpu, vxo, w, cams, okw, multi=multi, common=common)
            assert counter == expect > 0
            assert bounce > counter


def test_sample_start_outside_the_grid_keeps_the_ray_finished_phase(gpu, vxo, worlds):
    """Solid voxels in the top layer and along the +x and +z faces, seen from outside and above, lit from below so that those
    outer faces are shadowed: position + normal * 0.01f of a hit on one of them lies outside the grid, and that lane must be
    left to the ray-finished phase; shadowed hits inside the grid take the hook."""
    w = worlds["edge"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, [((75.0, 85.0, 25.0), (35.0, 10.0, 30.0)), ((30.0, 80.0, 85.0), (30.0, 10.0, 35.0))])
    light = (-0.5, -0.7, -0.5)
    expect, shadowed = _expected(vxo, w, "edge", cams, [3, 4], light=light)
    assert 100 < expect < shadowed - 100
    for multi in (False, True):
        counter, _ = _check(gpu, vxo, w, cams, BENCH, multi=multi, light=light)
        assert counter == expect


@pytest.mark.parametrize("name,okw,kw", [
    ("hit-index AOV", BENCH, dict(hit_views=(0, 1))),
    ("hit-index AOV of one view", BENCH, dict(hit_views=(1,), multi=True)),
    ("no shadow", dict(shadow=False, bounce_samples=1), {}),
    ("debug view", dict(mode=1, shadow=True, bounce_samples=1), {}),
    ("no bounce samples", dict(shadow=True, bounce_samples=0), {}),
    ("second bounce", dict(shadow=True, bounce_samples=2, bounce_depth=2), {}),
    ("axis light", BENCH, dict(light=(0.0, 1.0, 0.0))),
    ("light with a component below 2^-40", BENCH, dict(light=(0.6, 1e-13, 0.8))),
])
def test_path_off(gpu, vxo, worlds, name, okw, kw):
    """Launches the continuation must leave alone (counter 0, frames equal): the ones the launch flag excludes, and the
    second-bounce instantiations, which are compiled without it."""
    w = worlds["interior"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, sfe.INTERIOR_CAMS[:2])
    for multi in ((True,) if kw.get("multi") else (False, True)):
        counter, _ = _check(gpu, vxo, w, cams, okw, **{**kw, "multi": multi})
        assert counter == 0


def test_a_light_that_is_not_finite_is_refused(gpu):
    """The launch flag's finite-light condition cannot be reached through the API: SetEnvironment refuses such a light."""
    vx, ctx, torch = gpu
    for light in ((float("inf"), 1.0, 1.0), (0.5, float("nan"), 0.5)):
        with pytest.raises(vx.VxrtError):
            ctx.SetEnvironment(light, (2, 2, 2), (0.5, 0.5, 0.5))


def test_checkerboard_and_orthographic_launches_keep_the_path(gpu, vxo, worlds):
    """General-instantiation options that change which pixels exist or how their rays start, not the continuation."""
    w = worlds["interior"]
    helpers.upload(gpu[1], w)
    cams = _view_cams(vxo, sfe.INTERIOR_CAMS[:2])
    for okw in (dict(shadow=True, bounce_samples=1, checkerboard=True), dict(shadow=True, bounce_samples=1, ortho=True)):
        for multi in (False, True):
            counter, bounce = _check(gpu, vxo, w, cams, okw, multi=multi)
            assert 0 < counter <= bounce


def test_strip_shards_reassemble(gpu, vxo, worlds):
    """Strip sharding with compact shard buffers: the shards reassemble to the oracle's frame and their counters -- the new one
    included -- add up to the whole frame's."""
    vx, ctx, torch = gpu
    w = worlds["interior"]
    helpers.upload(ctx, w)
    ctx.SetEnvironment((INV, INV, INV), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    cam = _view_cams(vxo, sfe.INTERIOR_CAMS[:1])
    want, rays, probes = sfe._oracle(vxo, w, cam, BENCH, [3], (INV, INV, INV), False)
    expect, _ = _expected(vxo, w, "interior", cam, [3])
    pos, f, u, r = cam[0]
    rows, count = 8, 3
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
                assert ctx.loop_counters()["end_bounce"] == expect > 0
        finally:
            ctx.set_kernel_variant(4)


def test_temporal_accumulation(gpu, vxo, worlds):
    """Temporal accumulation (single-view launches): frames and histories of three frames with a reset equal the oracle's; the
    shaded colour the hook takes from the wave's table reaches the history in the ray-finished phase as before."""
    vx, ctx, torch = gpu
    w = worlds["interior"]
    helpers.upload(ctx, w)
    ctx.SetEnvironment((INV, INV, INV), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    cam = _view_cams(vxo, sfe.INTERIOR_CAMS[:1])
    pos, f, u, r = cam[0]
    for variant, stats in ((4, False), (4, True), (1, False)):
        ctx.set_kernel_variant(variant)
        try:
            acc_c, fb_c = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.uint8)
            acc_g = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            fb_g = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            for frame in range(1, 4):
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
                    assert ctx.loop_counters()["end_bounce"] == _expected(vxo, w, "interior", cam, [frame])[0] > 0
        finally:
            ctx.set_kernel_variant(4)


def test_wide_grid(gpu, vxo):
    """A coarse grid beyond the tracer's packed step counters (1024 cells along x, 8 x 8 across): the wide-grid instantiations,
    whose start_walk also arms the CF_OFF_* words for the walks the hook records."""
    rng = np.random.default_rng(1024)
    X = 1024 * 8
    v = np.zeros((X, 64, 64), bool)
    n_vox = int(X * 64 * 64 * 0.00003)
    v[rng.integers(0, X, n_vox), rng.integers(0, 64, n_vox), rng.integers(0, 64, n_vox)] = True
    v[:, 0, :] = True
    v[4090:4110, 1:30, 28:36] = True  # a shadow caster in front of the second camera
    w = vxo.World.from_voxels(v, 8)
    assert w.cdims[0] == 1024
    helpers.upload(gpu[1], w)
    cams = [helpers.camera("A", w.dims, vxo), sfe._cam(vxo, (4000.0, 40.0, 30.0), (4100.0, 0.0, 32.0))]
    expect, _ = _expected(vxo, w, "wide", cams, [3, 4])
    assert expect > 0
    for multi in (False, True):
        counter, _ = _check(gpu, vxo, w, cams, BENCH, multi=multi)
        assert counter == expect
