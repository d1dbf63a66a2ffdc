"""The HIP path against the REFERENCE'S OWN CODE, live: the host-compiled reference libraries (oracle/_ref, built by
__graft_entry__.build() where the reference's sources are; they travel with the tree) run next to the GPU.  Worlds are
built by the reference's builder and uploaded from ITS tables, rays and frames go through both, and every output must be
equal bit for bit.  Nothing here reads the reference's sources; the tests skip only where oracle/_ref is absent.
tests/test_ref_golden.py holds the recorded counterpart that never skips."""
import numpy as np
import pytest

from tests import helpers, ref_pin_cases as P, render_edge_cases as rec

pytestmark = pytest.mark.gpu
fb = helpers.float_bits


@pytest.fixture(scope="module")
def vxref():
    from oracle import vxref as m
    if not m.available():
        pytest.skip("oracle/_ref is absent or older than the recipe (it is built where the reference's sources are)")
    return m


@pytest.fixture(scope="module")
def eng():
    import torch
    import voxelengine_amd as vx
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return vx, torch


def _upload(ctx, ref_world):
    ctx.upload_world(*ref_world.engine_tables())


def _opts(vx, sw, n):
    return vx.RenderOptions(mode=sw.get("mode", 0), checkerboard=bool(sw.get("checkerboard", 0)), shadow=bool(sw.get("shadow", 0)),
                            bounce_samples=sw.get("bounce_samples", 0), ortho=bool(sw.get("ortho", 0)), frame_number=n)


def _reference_frame(r, p, n, fbuf):
    return r.render(p.width, p.height, n, p.origin[:], p.fwd[:], p.up[:], p.right[:], fb=fbuf, fov=p.fov_deg, ortho_size=p.ortho_size[:],
                    light_dir=p.env.light_dir[:], light_color=p.env.light_color[:], ambient=p.env.ambient[:])


def test_batches(eng, vxref):
    vx, _ = eng
    name = "random16"
    r = P.reference_world(name, vxref.DEFAULT)
    # The default context gets the issue's 30k rays: one ray per lane (k_trace_batch_wave2).  The queue kernel
    # (k_trace_batch_persist) takes a batch of at least 8 rays per lane of the persistent grid (launch_trace_batch,
    # vxrt_kernels.hip): with one persistent wave per CU on 256 CUs that is 8 * 64 * 256 = 131072 rays, so the small-grid
    # context gets 262145 -- the size tests/test_gpu_parity.py::test_trace_batch_persistent_queue uses -- with a ragged
    # last ticket.  Kernel variant 1 runs the cross-check loops on either context.
    for waves, n in ((0, 30000), (1, 262145)):
        o, d = P.mixed_rays(P.WORLDS[name][0], n)
        assert rec._valid(o, d).all()
        want = {ms: r.trace(o, d, ms) for ms in (2048, 8)}
        assert 0 < int(want[2048]["hit"].sum()) < len(o) and not np.array_equal(want[2048]["steps"], want[8]["steps"])
        ctx = helpers.new_ctx(vx)
        try:
            if waves:
                ctx.set_persistent_waves_per_cu(waves)
            _upload(ctx, r)
            for kv in (4, 1):
                ctx.set_kernel_variant(kv)
                for ms in (2048, 8):
                    ctx.set_batch_max_steps(ms)
                    for stats in (False, True):
                        g = ctx.Raytrace(o, d, want_stats=stats)
                        what = (waves, kv, ms, stats)
                        assert np.array_equal(g["hit"], want[ms]["hit"]) and np.array_equal(g["steps"], want[ms]["steps"]), what
                        assert np.array_equal(fb(g["normal"]), fb(want[ms]["normal"])), what
                        assert np.array_equal(fb(g["hitPoint"]), fb(want[ms]["pos"])), what
        finally:
            ctx.close()


@pytest.mark.parametrize("variant", list(__import__("oracle.ref_build", fromlist=["VARIANTS"]).VARIANTS))
def test_frames(eng, vxref, variant):
    vx, torch = eng
    sw = vxref.switches(variant)
    r = P.reference_world("terrain32", variant)
    ctx = helpers.new_ctx(vx)
    try:
        _upload(ctx, r)
        for cam in "AD":
            camera = P.frame_camera(cam, r.dims)
            ref_fb = np.full((P.FRAME_H, P.FRAME_W, 4), 77, np.uint8)
            gpu_fb = {kv: torch.full((P.FRAME_H, P.FRAME_W, 4), 77, dtype=torch.uint8, device="cuda") for kv in (4, 1)}
            for n in P.FRAME_NUMBERS:
                p = P.make_params(P.FRAME_W, P.FRAME_H, camera, sw, n)
                _reference_frame(r, p, n, ref_fb)
                ctx.SetOrthoWindowSize(*p.ortho_size[:])
                for kv in (4, 1):
                    ctx.set_kernel_variant(kv)
                    ctx.RenderScreen(P.FRAME_W, P.FRAME_H, gpu_fb[kv], *camera, _opts(vx, sw, n))
                    got = gpu_fb[kv].cpu().numpy()
                    bad = np.argwhere((got != ref_fb).any(axis=2))
                    assert bad.size == 0, (variant, cam, n, kv, len(bad), bad[:3])
    finally:
        ctx.close()


def test_facade_views(eng, vxref):
    """one RenderViews launch of the four cameras against four reference frames (shadow trace and one bounce sample)"""
    vx, torch = eng
    variant = "shadow_s1"
    sw = vxref.switches(variant)
    r = P.reference_world("terrain32", variant)
    ctx = helpers.new_ctx(vx)
    try:
        _upload(ctx, r)
        views, want = [], []
        for i, cam in enumerate("ABCD"):
            camera = P.frame_camera(cam, r.dims)
            n = i                                                   # frame numbers 0..3: both checkerboard parities
            p = P.make_params(P.FRAME_W, P.FRAME_H, camera, sw, n)
            want.append(_reference_frame(r, p, n, np.full((P.FRAME_H, P.FRAME_W, 4), 77, np.uint8)))
            views.append(dict(fb=torch.full((P.FRAME_H, P.FRAME_W, 4), 77, dtype=torch.uint8, device="cuda"), origin=camera[0],
                              fwd=camera[1], up=camera[2], right=camera[3], frame_number=n))
        ctx.RenderViews(P.FRAME_W, P.FRAME_H, views, _opts(vx, sw, 0))
        for cam, v, w in zip("ABCD", views, want):
            assert np.array_equal(v["fb"].cpu().numpy(), w), cam
    finally:
        ctx.close()
