"""The render edge cases (tests/render_edge_cases.py) reach what they name: every case renders with the oracle, at least one
pixel meets each of the case's target branches (the oracle's per-pixel census, oracle/vxo.h VXO_CEN_*), and no camera,
shadow or bounce ray of the frame is invalid (include/vxrt.h) -- checked both by the census and by a binary32 numpy
restatement of the camera ray over every pixel and of the light's unit vector.  The render kernel has no ray_valid guard,
so a case that handed it an invalid ray would be a bug in the table."""
import numpy as np
import pytest

from tests import render_edge_cases as rc


@pytest.mark.parametrize("case", rc.CASES, ids=rc.CASE_IDS)
def test_edge_case_reaches_its_target_with_valid_rays(vxo, case):
    assert rc.camera_rays_valid(case), case
    assert rc.light_valid(case.env["light_dir"]), case
    w = rc.world(vxo, case.world)
    out = w.render(case.params(vxo), want_census=True, nthreads=16)
    cen = out["census"]
    assert not (cen & vxo.CEN_INVALID).any(), case
    met = {name: int(((cen & getattr(vxo, "CEN_" + name)) != 0).sum()) for name in case.targets}
    assert all(met.values()), (case, met)
    assert out["stats"].primary_hits > 0, case


def test_census_changes_no_result(vxo):
    """the census is bookkeeping: a frame with it equals the frame without it, byte for byte, AOVs and counters included"""
    case = next(c for c in rc.CASES if c.name == "light_axis_view_axis")
    w = rc.world(vxo, case.world)
    fb0 = np.random.default_rng(5).integers(0, 255, size=(case.H, case.W, 4), dtype=np.uint8)
    a = w.render(case.params(vxo), fb=fb0.copy(), want_color=True, want_hit=True)
    b = w.render(case.params(vxo), fb=fb0.copy(), want_color=True, want_hit=True, want_census=True)
    assert np.array_equal(a["fb"], b["fb"]) and np.array_equal(a["hit"], b["hit"])
    assert np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32))
    assert a["stats"].total_rays() == b["stats"].total_rays() and a["census"] is None
    assert (b["census"] & (vxo.CEN_SPECIAL_PRIMARY | vxo.CEN_SPECIAL_SHADOW)).any()


def test_ordinary_frames_meet_no_edge_branch(vxo):
    """the census is not trivially true: camera A with the default environment meets none of the fall-backs and no special
    primary or shadow ray"""
    from tests import helpers
    w = rc.world(vxo, "terrain32")
    pos, f, u, r = helpers.camera("A", w.dims, vxo)
    out = w.render(vxo.make_params(64, 48, pos, f, u, r, shadow=1, bounce_samples=1, frame_number=3), want_census=True)
    assert not (out["census"] & ~np.uint8(vxo.CEN_SPECIAL_BOUNCE)).any()


def test_invalid_rays_are_flagged(vxo):
    """the validity checks themselves: a camera whose fwd, up and right are 0 and a zero light are refused"""
    c = rc.Case("zero_camera", "random8", (), (1, 2, 3), (0, 0, 0), (0, 0, 0), (0, 0, 0))
    assert not rc.camera_rays_valid(c)
    out = rc.world(vxo, "random8").render(c.params(vxo), want_census=True)
    assert (out["census"] & vxo.CEN_INVALID).all()
    assert not rc.light_valid((0, 0, 0)) and not rc.light_valid((1e-30, 0, 0)) and not rc.light_valid((np.inf, 0, 0))
    assert rc.light_valid((3, 4, 0)) and rc.light_valid((1e-13, 1, 0))


@pytest.mark.parametrize("seed", range(40))
def test_random_edge_frames_are_valid(vxo, seed):
    """the fuzz tool's edge-case generator (tests/tools/fuzz_parity.py) only makes valid frames"""
    rng = np.random.default_rng(seed)
    w = rc.world(vxo, "random8")
    cam = rc.random_axis_camera(rng, w.dims)
    env, fov = rc.random_environment(rng)
    c = rc.Case("random", "random8", (), *cam, fov=fov, env=env, ortho=int(rng.integers(0, 2)), ortho_size=(32, 32))
    assert rc.camera_rays_valid(c) and rc.light_valid(env["light_dir"])
    out = w.render(c.params(vxo), want_census=True)
    assert not (out["census"] & vxo.CEN_INVALID).any()
