"""GPU parity on the render edge cases (tests/render_edge_cases.py): axis-aligned views and lights, ortho views on grid
lines, tiny and wide FOVs, camera vectors far from unit length, a camera inside a solid voxel, colours far from 1.  Every
case's frame (stale contents kept), colour AOV (NaN / inf positions included), hit AOV, ray counters and probe counters
equal the oracle's, from the timed and the probe-counting instantiation of the persistent render kernel (7) and from the
cross-check kernel (1); axis-aligned views share one multi-view launch with camera A; the wide-grid case runs the WIDE
instantiation, the cases with bounce_depth 2 the BOUNCE2 one.  The census test (tests/test_render_edge_census.py) proves
on the oracle that each case reaches the branch it names."""
import numpy as np
import pytest

from tests import render_edge_cases as rc
from tests.helpers import upload
from tests.test_gpu_parity import _assert_frame_equal, _render_both, eng  # noqa: F401  (eng: the module's context)

pytestmark = pytest.mark.gpu


def _uploaded(eng, vxo, name):
    """the case world, uploaded unless it is the one the context holds already"""
    _, ctx, _ = eng
    w = rc.world(vxo, name)
    if getattr(ctx, "_edge_world", None) != name:
        upload(ctx, w)
        ctx._edge_world = name
    return w


@pytest.mark.parametrize("case", rc.CASES, ids=rc.CASE_IDS)
def test_edge_case_frame_equals_the_oracle(eng, vxo, case):
    vx, ctx, _ = eng
    w = _uploaded(eng, vxo, case.world)
    default = ctx.kernel_variant
    try:
        for variant in (7, 1):   # _render_both asserts that the launch runs the variant that is set
            ctx.set_kernel_variant(variant)
            cpu, fb, col, hit, st = _render_both(eng, vxo, w, case.W, case.H, case.camera, **case.render_kw())
            _assert_frame_equal(cpu, fb, col, hit, st)
            assert st.primary_hits > 0
    finally:
        ctx.set_kernel_variant(default)


def test_axis_views_share_a_multi_view_launch_with_camera_a(eng, vxo):
    """One vxrt_render_views launch (the MULTI instantiation) of axis-aligned views -- special lanes -- and camera A --
    ordinary lanes -- in the same waves: every view equals the oracle, frame (stale contents kept) and hit AOV, and the
    launch traces the oracle's rays."""
    vx, ctx, torch = eng
    w = _uploaded(eng, vxo, "terrain32")
    names = ["opening_view", "view_nx", "euler_zero", "view_py_from_below", "euler_plus_half_pi", "fwd_component_1e-30"]
    cases = [c for c in rc.CASES if c.name in names]
    assert len(cases) == len(names) and all(c.env == rc.DEFAULT_ENV and c.fov == 90.0 and not c.ortho for c in cases)
    cams = [c.camera for c in cases]
    cams.insert(3, (rc.POS_A, rc.FA, rc.UA, rc.RA))
    W, H = 64, 48
    opts = vx.RenderOptions(shadow=True, bounce_samples=1)
    ctx.SetEnvironment(rc.DEFAULT_ENV["light_dir"], rc.DEFAULT_ENV["light_color"], rc.DEFAULT_ENV["ambient"])
    ctx.SetFOV(90.0)
    assert ctx.kernel_for_launch(W, H, opts, nviews=len(cams)) == 7
    fb0 = np.random.default_rng(9).integers(0, 255, size=(H, W, 4), dtype=np.uint8)
    views, wants, rays = [], [], 0
    for j, cam in enumerate(cams):
        p = vxo.make_params(W, H, *cam, frame_number=5 + j, shadow=1, bounce_samples=1)
        want = w.render(p, fb=fb0.copy(), want_hit=True)
        wants.append(want)
        rays += want["stats"].total_rays()
        views.append(dict(fb=torch.from_numpy(fb0.copy()).cuda(), origin=cam[0], fwd=cam[1], up=cam[2], right=cam[3],
                          frame_number=5 + j, hit_aov=torch.full((H, W), -7, dtype=torch.int64, device="cuda")))
    ctx.frame_stats()
    ctx.RenderViews(W, H, views, opts)
    assert ctx.frame_stats().total_rays() == rays
    for j, (v, want) in enumerate(zip(views, wants)):
        assert np.array_equal(v["fb"].cpu().numpy(), want["fb"]), j
        assert np.array_equal(v["hit_aov"].cpu().numpy(), want["hit"]), j


def test_degenerate_light_is_refused_and_the_environment_kept(eng, vxo):
    """vxrt_set_environment refuses a light_dir with a non-finite component or a binary32 squared length of 0 or
    infinity (include/vxrt.h); the context keeps the environment it had, and the next frame equals the oracle's with it."""
    vx, ctx, torch = eng
    w = _uploaded(eng, vxo, "random8")
    case = next(c for c in rc.CASES if c.name == "neg_zero_origin_oblique")
    env = dict(light_dir=(3.0, 4.0, 0.0), light_color=(1.5, 2.0, 2.5), ambient=(0.25, 0.5, 0.75))
    ctx.SetEnvironment(env["light_dir"], env["light_color"], env["ambient"])
    nan, inf = float("nan"), float("inf")
    for bad in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (nan, 1.0, 0.0), (0.0, inf, 0.0), (1.0, 0.0, -inf), (1e-30, 0.0, 0.0),
                (1e-23, 1e-23, 1e-23), (1e20, 0.0, 0.0), (2e19, 2e19, 2e19)):
        with pytest.raises(vx.VxrtError):
            ctx.SetEnvironment(bad, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    for ok in ((1e-19, 0.0, 0.0), (1e19, 0.0, 0.0), (0.0, 1e-13, 0.0)):   # small or large, but a finite unit vector
        ctx.SetEnvironment(ok, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    ctx.SetEnvironment(env["light_dir"], env["light_color"], env["ambient"])
    with pytest.raises(vx.VxrtError):   # refused: nothing of it is taken, colour and ambient included
        ctx.SetEnvironment((0.0, 0.0, 0.0), (9.0, 9.0, 9.0), (9.0, 9.0, 9.0))
    W, H = case.W, case.H
    p = vxo.make_params(W, H, *case.camera, frame_number=2, shadow=1, bounce_samples=1, **env)
    want = w.render(p, fb=np.zeros((H, W, 4), np.uint8))["fb"]
    ctx.SetFOV(90.0)
    ctx.SetOrthoWindowSize(10.0, 10.0)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.RenderScreen(W, H, fb, *case.camera, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=2))
    assert np.array_equal(fb.cpu().numpy(), want)
