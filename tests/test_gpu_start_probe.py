"""The round order of the persistent render kernel built on the probed coarse set-up (voxelengine_amd/csrc/vxrt_persist2.hpp,
vxrt_wave2.hpp: start_pending_probed): end-of-walk phase, ray-finished phase, ONE set-up of the coarse walks both recorded
that also runs their first probe, then the tight-box phase -- which so takes a lane whose walk starts in an occupied coarse
cell in the round that set it up -- then the probe burst.  A schedule changes no result: every case compares the timed and
the counting instantiation of the product kernel, on a persistent grid shrunk to one wave per CU so that lanes are reused,
with the CPU oracle: frame buffers and hit indices byte for byte, the colour AOV within 1e-4, the four ray counters and
the three probe counters.  The worlds are the golden ones (tests/golden/make_golden.py), the same terrain at brick edge 32
(the COMMON instantiations run on no other edge) and a 1024-cell-wide grid (the WIDE ones)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
make_golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_golden)

W, H = 96, 64
INV = helpers.INV
LIGHT = (INV, INV, INV)
COLOR_TOL = 1e-4
ORTHO = (60.0, 60.0)
BENCH = dict(shadow=True, bounce_samples=1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import voxelengine_amd as vx
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ctx = helpers.new_ctx(vx)
    ctx.set_persistent_waves_per_cu(1)
    yield vx, ctx, torch
    ctx.close()


@pytest.fixture(scope="module")
def worlds(vxo):
    return {"terrain": make_golden.world_terrain(), "sparse": make_golden.world_sparse(),
            "terrain32": vxo.World.generate(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32)}


def _cam(pos, target, up=(0.0, 1.0, 0.0)):
    """a camera at `pos` that looks at `target`: (origin, fwd, up, right), an orthonormal frame in binary32"""
    f = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    as32 = lambda v: tuple(float(np.float32(c)) for c in v)
    return (as32(pos), as32(f), as32(u), as32(r))


def _occupied_cells(w):
    """the occupied coarse cells (x, y, z) of an oracle world: brick_slot is in the reference's tiled cell order"""
    cx, cy, cz = (int(v) for v in w.cdims)
    occ = np.asarray(w.brick_slot) != 0xFFFFFFFF
    return [(x, y, z) for z in range(cz) for y in range(cy) for x in range(cx) if occ[_tiled(x, y, z, cx // 8, cy // 8)]]


def _tiled(x, y, z, tx, ty):
    """the reference's tiled cell order: 8 x 8 x 8 tiles, x fastest inside a tile and among tiles"""
    return ((x >> 3) + tx * ((y >> 3) + ty * (z >> 3))) * 512 + (x & 7) + 8 * ((y & 7) + 8 * (z & 7))


def _check(gpu, vxo, w, cams, okw, *, multi=False, hit_views=(), light=LIGHT, specialisation=None):
    """the timed and the counting launch of `cams` against the oracle; returns the oracle's ray counters"""
    vx, ctx, torch = gpu
    frame_numbers = [3 + k for k in range(len(cams))]
    ctx.SetEnvironment(light, (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    ctx.SetOrthoWindowSize(*ORTHO)
    ckw = dict(mode=0, checkerboard=0, shadow=int(okw.get("shadow", False)), bounce_samples=okw.get("bounce_samples", 0),
               bounce_all_hits=int(okw.get("bounce_all_hits", False)), ortho=int(okw.get("ortho", False)),
               bounce_depth=okw.get("bounce_depth", 1), ortho_size=ORTHO, light_dir=light)
    want, rays, probes = [], np.zeros(4, np.int64), np.zeros(3, np.int64)
    for (pos, f, u, r), fn in zip(cams, frame_numbers):
        out = w.render(vxo.make_params(W, H, pos, f, u, r, frame_number=fn, **ckw), fb=np.zeros((H, W, 4), np.uint8), want_color=True,
                       want_hit=True, nthreads=16)
        st = out["stats"]
        rays += (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits)
        probes += (st.probes.coarse_probes, st.probes.brick_entries, st.probes.fine_probes)
        want.append(out)
    if specialisation is not None:
        probe = torch.zeros(1, dtype=torch.int64, device="cuda") if hit_views else None
        assert ctx.render_specialisation(W, H, vx.RenderOptions(**okw), nviews=len(cams) if multi else 0, hit_aov=probe) == specialisation
    for stats in (False, True):
        fbs = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in cams]
        cols = [torch.full((H, W, 3), -3.0, dtype=torch.float32, device="cuda") for _ in cams]
        hits = [torch.full((H, W), -7, dtype=torch.int64, device="cuda") if k in hit_views else None for k in range(len(cams))]
        ctx.frame_stats()
        if multi:
            opts = vx.RenderOptions(collect_stats=stats, **okw)
            assert ctx.kernel_for_launch(W, H, opts, nviews=len(cams)) == 7
            ctx.RenderViews(W, H, [dict(fb=fbs[k], origin=c[0], fwd=c[1], up=c[2], right=c[3], frame_number=frame_numbers[k], color_aov=cols[k],
                                        hit_aov=hits[k]) for k, c in enumerate(cams)], opts)
        else:
            for k, c in enumerate(cams):
                opts = vx.RenderOptions(collect_stats=stats, frame_number=frame_numbers[k], **okw)
                assert ctx.kernel_for_launch(W, H, opts) == 7
                ctx.RenderScreen(W, H, fbs[k], c[0], c[1], c[2], c[3], opts, color_aov=cols[k], hit_aov=hits[k])
        st = ctx.frame_stats()
        for k in range(len(cams)):
            assert np.array_equal(fbs[k].cpu().numpy(), want[k]["fb"]), (stats, k)
            if hits[k] is not None:
                assert np.array_equal(hits[k].cpu().numpy(), want[k]["hit"]), (stats, k)
            col, ref = cols[k].cpu().numpy(), want[k]["color"]
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(col), fin), (stats, k)
            assert np.max(np.abs(col[fin] - ref[fin]), initial=0.0) <= COLOR_TOL, (stats, k)
        assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == tuple(int(v) for v in rays), stats
        if stats:
            assert (st.coarse_probes, st.brick_entries, st.fine_probes) == tuple(int(v) for v in probes)
            assert st.guard_stray_loads == 0
    return rays


@pytest.mark.parametrize("world", ["terrain", "sparse"])
def test_cameras_inside_occupied_coarse_cells(gpu, vxo, worlds, world):
    """Every primary ray starts in an occupied coarse cell: the set-up's probe parks the whole launch for the tight-box phase."""
    w = worlds[world]
    helpers.upload(gpu[1], w)
    cells = _occupied_cells(w)
    assert cells
    cams = []
    for pick, off in ((len(cells) // 3, (0.5, 0.5, 0.5)), (2 * len(cells) // 3, (0.25, 0.7, 0.4))):
        x, y, z = cells[pick]
        pos = tuple((c + o) * w.factor for c, o in zip((x, y, z), off))
        cams.append(_cam(pos, tuple(0.5 * d + 3.0 for d in w.dims)))
    for multi in (False, True):  # (two views in one launch)
        rays = _check(gpu, vxo, w, cams, BENCH, multi=multi)
        assert rays[0] == 2 * W * H and rays[3] > 0


@pytest.mark.parametrize("world", ["terrain", "sparse"])
def test_cameras_on_the_far_faces_looking_in(gpu, vxo, worlds, world):
    """Origins exactly on the +x, +y and +z faces, on two of them and on the far corner."""
    w = worlds[world]
    helpers.upload(gpu[1], w)
    X, Y, Z = (float(d) for d in w.dims)
    mid = (0.5 * X + 1.0, 0.4 * Y, 0.5 * Z - 1.0)
    cams = [_cam((X, 0.55 * Y, 0.45 * Z), mid), _cam((0.45 * X, Y, 0.55 * Z), mid, up=(0.0, 0.0, 1.0)), _cam((0.5 * X, 0.6 * Y, Z), mid),
            _cam((X, Y, 0.5 * Z), mid), _cam((X, Y, Z), mid)]
    rays = _check(gpu, vxo, w, cams, BENCH)
    assert rays[3] > 0
    _check(gpu, vxo, w, cams[2:], BENCH, multi=True)


@pytest.mark.parametrize("light", [(0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.6, 1e-13, 0.8)])
def test_axis_aligned_lights(gpu, vxo, worlds, light):
    """Every shadow ray is `special`: set up in single-step mode, so the set-up's probe ends or parks every one of them."""
    w = worlds["terrain"]
    helpers.upload(gpu[1], w)
    cams = [_cam((100.0, 110.0, 20.0), (60.0, 30.0, 70.0)), _cam((20.5, 90.0, 100.25), (64.0, 40.0, 64.0))]
    for multi in (False, True):
        rays = _check(gpu, vxo, w, cams, BENCH, multi=multi, light=light)
        assert rays[1] == rays[3] > 0


@pytest.mark.parametrize("world", ["terrain", "sparse"])
def test_orthographic_axis_aligned_views(gpu, vxo, worlds, world):
    """Orthographic cameras that look straight down and along -x: every primary ray has two zero components (general
    instantiation, `special` rays), from origins above and beside the grid and inside it."""
    w = worlds[world]
    helpers.upload(gpu[1], w)
    X, Y, Z = (float(d) for d in w.dims)
    down = lambda pos: (pos, (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    along = lambda pos: (pos, (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    cams = [down((0.5 * X, Y + 10.0, 0.5 * Z)), down((0.5 * X + 0.25, 0.75 * Y, 0.5 * Z)), along((X + 5.0, 0.5 * Y, 0.5 * Z)),
            along((0.6 * X, 0.5 * Y + 0.5, 0.5 * Z))]
    okw = dict(ortho=True, **BENCH)
    rays = _check(gpu, vxo, w, cams, okw)
    assert rays[3] > 0
    _check(gpu, vxo, w, cams[:2], okw, multi=True)


@pytest.mark.parametrize("multi", [False, True], ids=["single view", "two views"])
def test_plain_launch_and_the_same_forced_general(gpu, vxo, worlds, multi):
    """Brick edge 32: the plain shaded launch runs a COMMON instantiation, the same launch with a hit-index AOV the general
    one (which then also launches its shadow rays from the ray-finished phase instead of the end-of-walk phase's hook)."""
    w = worlds["terrain32"]
    helpers.upload(gpu[1], w)
    cams = [helpers.camera("A", w.dims, vxo), helpers.camera("C", w.dims, vxo)]
    plain = _check(gpu, vxo, w, cams, BENCH, multi=multi, specialisation=1)
    general = _check(gpu, vxo, w, cams, BENCH, multi=multi, hit_views=(0, 1), specialisation=0)
    assert tuple(plain) == tuple(general) and plain[3] > 0


@pytest.mark.parametrize("name,okw", [
    ("no shadow", dict(shadow=False, bounce_samples=1)),
    ("no shadow, no samples", dict(shadow=False, bounce_samples=0)),
    ("no samples", dict(shadow=True, bounce_samples=0)),
    ("two samples", dict(shadow=True, bounce_samples=2)),
    ("two samples, all hits", dict(shadow=True, bounce_samples=2, bounce_all_hits=True)),
    ("second bounce", dict(shadow=True, bounce_samples=2, bounce_depth=2, bounce_all_hits=True)),
])
@pytest.mark.parametrize("world", ["terrain", "terrain32"])
def test_ray_chains(gpu, vxo, worlds, world, name, okw):
    """shadow = 0, bounce_samples 0 and 2, bounce_depth = 2, one view per launch and two views in one (the general multi-view
    second-bounce instantiation keeps the earlier round order: box, end, next, plain set-up)."""
    w = worlds[world]
    helpers.upload(gpu[1], w)
    cams = [helpers.camera("A", w.dims, vxo), helpers.camera("D", w.dims, vxo)]
    for multi in (False, True):
        rays = _check(gpu, vxo, w, cams, okw, multi=multi)
        assert rays[3] > 0 and (rays[1] > 0) == okw["shadow"] and (rays[2] > 0) == (okw["bounce_samples"] > 0)


def test_wide_grid(gpu, vxo):
    """A 1024-cell-wide grid at brick edge 8 (the WIDE instantiations: the set-up's probe also tests rem's guard bits), with
    cameras inside occupied cells of the floor, above it and on the far +x face."""
    rng = np.random.default_rng(1024)
    X = 1024 * 8
    v = np.zeros((X, 64, 64), bool)
    n_vox = int(X * 64 * 64 * 0.00003)
    v[rng.integers(0, X, n_vox), rng.integers(0, 64, n_vox), rng.integers(0, 64, n_vox)] = True
    v[:, 0, :] = True
    w = vxo.World.from_voxels(v, 8)
    assert w.cdims[0] == 1024
    helpers.upload(gpu[1], w)
    cams = [helpers.camera("A", w.dims, vxo), _cam((4000.0, 40.0, 30.0), (4100.0, 0.0, 32.0)), _cam((4003.5, 4.5, 20.5), (4100.0, 30.0, 40.0)),
            _cam((float(X), 30.0, 32.0), (float(X) - 200.0, 0.0, 30.0))]
    for multi in (False, True):
        rays = _check(gpu, vxo, w, cams, BENCH, multi=multi)
        assert rays[1] == rays[3] > 0
    _check(gpu, vxo, w, cams[:2], dict(shadow=True, bounce_samples=2, bounce_depth=2, bounce_all_hits=True), multi=True)
