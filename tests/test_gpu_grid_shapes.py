"""The grid shapes of tests/grid_shape_cases.py on the device: grids long in y and in z, the largest ordinary grids, grids
wide by one disjunct of grid_is_wide alone, the ABI's largest dimension.  Per case, bit-equal to the oracle on the same
tables (tests/sparse_world.py), no tolerance except the colour AOV's of tests/test_gpu_parity.py:

1. the load guard first: the first tracing launch on the case's world counts its loads (the queue kernel with probe
   counters); none may be outside what the allocator made addressable, and some must be in the slack -- a stray index is
   then looked for on the host harness (tests/test_host_wave_logic.py), not by running again;
2. the tables come back from download_world unchanged (k_layout_bits, k_layout_meta, k_layout_bricks on these shapes);
3. batches of G.N_RAYS rays of G.rays(case) through the queue kernel (four permutations of them in one batch: at least 8
   rays per lane of a persistent grid of one wave per CU), one ray per lane and the straightforward loops, with and
   without probe counters: hit, steps, position bits, normal, 64-bit voxel index, probe counters;
4. the frames of G.views(case) through the persistent render kernel (timed and probe-counting instantiation) and the
   cross-check kernel, and all cameras of the case in one multi-view launch against their single-view frames;
5. on O2, W2 and W3 a region read straddling the far corner against the voxel list."""
import numpy as np
import pytest

from tests import grid_shape_cases as G
from tests.helpers import upload
from tests.test_gpu_parity import _assert_batch_equal, _assert_frame_equal

pytestmark = pytest.mark.gpu

W, H = G.FRAME_W, G.FRAME_H
REGION_CASES = ("O2", "W2", "W3")


@pytest.fixture(scope="module")
def eng():
    import torch
    import voxelengine_amd as vx
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ctx = vx.Context(0)
    small = vx.Context(0)
    small.set_persistent_waves_per_cu(1)   # a small persistent grid: 4 * G.N_RAYS rays take the queue kernel
    yield vx, ctx, small, torch
    ctx.close()
    small.close()


def _probes(st):
    return (st.coarse_probes, st.brick_entries, st.fine_probes)


def _render(vx, ctx, torch, cam, kw, fb0, variant, collect_stats=False, aov=True):
    okw = dict(shadow=True, bounce_samples=1, frame_number=G.FRAME_NUMBER, ortho=bool(kw.get("ortho", 0)), collect_stats=collect_stats)
    opts = vx.RenderOptions(**okw)
    assert ctx.kernel_for_launch(W, H, opts) == variant
    fb = torch.from_numpy(fb0.copy()).cuda()
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") if aov else None
    hit = torch.full((H, W), -1, dtype=torch.int64, device="cuda") if aov else None
    ctx.frame_stats()   # counters accumulate until read: start this frame from zero
    ctx.RenderScreen(W, H, fb, *cam, opts, color_aov=col, hit_aov=hit)
    st = ctx.frame_stats()
    return fb.cpu().numpy(), col.cpu().numpy() if aov else None, hit.cpu().numpy() if aov else None, st


def _set_view(ctx, p):
    ctx.SetEnvironment(list(p.env.light_dir), list(p.env.light_color), list(p.env.ambient))
    ctx.SetFOV(p.fov_deg)
    ctx.SetOrthoWindowSize(p.ortho_size[0], p.ortho_size[1])


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_grid_shape_on_the_device(eng, vxo, name):
    vx, ctx, small, torch = eng
    case = G.BY_NAME[name]
    tables = G.tables(name)
    w = G.world(vxo, case)
    o, d, _ = G.rays(case, G.N_RAYS, case.seed)
    cpu = w.trace_batch(o, d, nthreads=16)
    assert int(cpu["steps"].max()) >= min(max(case.cells), 2048)
    want_probes = _probes(cpu["stats"])
    default = ctx.kernel_variant
    try:
        # ---- 1. the load guard, on the first tracing launch of this world
        upload(small, w)
        perm = np.concatenate([np.random.default_rng(case.seed + k).permutation(G.N_RAYS) for k in range(4)])
        oq, dq = np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm])
        g = small.Raytrace(oq, dq, want_stats=True)
        st = g["stats"]
        assert st.guard_stray_loads == 0, st.guard_stray_loads
        assert st.guard_slack_loads > 0
        cpu_q = {k: cpu[k][perm] for k in ("hit", "steps", "voxel", "pos", "normal")}
        _assert_batch_equal(g, cpu_q)
        assert st.primary_rays == len(perm) and st.primary_hits == 4 * int(cpu["hit"].sum())
        assert _probes(st) == tuple(4 * v for v in want_probes)
        # ---- 2. the tables
        got = small.download_world()
        assert tuple(got["cdims"]) == case.cells and got["factor"] == case.factor
        for k, key in enumerate(("coarse_bits", "brick_slot", "bounds", "pool")):
            assert np.array_equal(got[key].view(np.uint32).reshape(-1), tables[k].view(np.uint32).reshape(-1)), key
        del got
        # ---- 3. batches: the queue kernel as timed; one ray per lane and the loops, counting and as timed
        _assert_batch_equal(small.Raytrace(oq, dq), cpu_q)
        del oq, dq, cpu_q, g
        upload(ctx, w)
        for variant in (4, 1):
            ctx.set_kernel_variant(variant)
            g = ctx.Raytrace(o, d, want_stats=True)
            _assert_batch_equal(g, cpu)
            assert g["stats"].guard_stray_loads == 0 and _probes(g["stats"]) == want_probes, variant
            _assert_batch_equal(ctx.Raytrace(o, d), cpu)
        # ---- 4. frames
        fb0 = np.random.default_rng(7).integers(0, 255, size=(H, W, 4), dtype=np.uint8)  # stale contents survive
        views = G.views(case)
        for v in views:
            p = vxo.make_params(W, H, *v["cam"], frame_number=G.FRAME_NUMBER, shadow=1, bounce_samples=1, **v["kw"])
            want = w.render(p, fb=fb0.copy(), want_color=True, want_hit=True, nthreads=16)
            assert want["stats"].primary_hits > 0 and want["stats"].shadow_rays > 0, v["name"]
            _set_view(ctx, p)
            for variant in (4, 1):
                ctx.set_kernel_variant(variant)
                kernel = 7 if variant == 4 else 1
                fb, col, hit, plain = _render(vx, ctx, torch, v["cam"], v["kw"], fb0, kernel)
                fb2, _, _, st = _render(vx, ctx, torch, v["cam"], v["kw"], fb0, kernel, collect_stats=True, aov=False)
                assert np.array_equal(fb2, fb), (v["name"], variant)
                assert plain.total_rays() == st.total_rays() and st.guard_stray_loads == 0, (v["name"], variant)
                _assert_frame_equal(want, fb, col, hit, st)
        # ... and every camera of the case in one launch (perspective, the default light) against its single-view frame
        ctx.set_kernel_variant(4)
        cams = [v["cam"] for v in views if v["name"].split("_")[0] != "light"]
        p = vxo.make_params(W, H, *cams[0], fov=G.VIEW_FOV)
        _set_view(ctx, p)
        opts = vx.RenderOptions(shadow=True, bounce_samples=1)
        assert ctx.kernel_for_launch(W, H, opts, nviews=len(cams)) == 7
        singles = [_render(vx, ctx, torch, cam, {}, fb0, 7)[::2] for cam in cams]
        mv = [dict(fb=torch.from_numpy(fb0.copy()).cuda(), origin=cam[0], fwd=cam[1], up=cam[2], right=cam[3], frame_number=G.FRAME_NUMBER,
                   hit_aov=torch.full((H, W), -1, dtype=torch.int64, device="cuda")) for cam in cams]
        ctx.RenderViews(W, H, mv, opts)
        for j, ((fb, hit), view) in enumerate(zip(singles, mv)):
            assert np.array_equal(view["fb"].cpu().numpy(), fb) and np.array_equal(view["hit_aov"].cpu().numpy(), hit), j
        # ---- 5. the query plumbing once on a grid that is not long in x
        if name in REGION_CASES:
            dims = np.array(case.dims)
            lo = dims - 20
            vox = G.scene_voxels(case)
            inside = vox[((vox >= lo) & (vox < dims)).all(1)] - lo
            want_region = np.zeros((40, 40, 40), bool)
            want_region[inside[:, 0], inside[:, 1], inside[:, 2]] = True
            assert want_region.any()
            assert np.array_equal(ctx.read_region_host(tuple(int(v) for v in lo), (40, 40, 40)), want_region)
    finally:
        ctx.set_kernel_variant(default)
        ctx.frame_stats()
        del w
