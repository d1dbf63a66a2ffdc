"""The persistent render kernel's instantiations for plain shaded frames (voxelengine_amd/csrc/vxrt_persist2.hpp: COMMON;
launch_is_common in vxrt_kernels.hip): a launch in shaded mode with a perspective camera, no checkerboard, no strips, no
accumulation history and no hit-index AOV, on an ordinary grid of brick edge 32, runs a kernel in which those flags are
compile-time constants.  It only lets the compiler see constants: frames, AOVs, hit indices and counters are
what the general instantiation produces, bit for bit.

Every case first asks Context.render_specialisation which instantiation a launch takes -- 1 for the plain launch, 0 for the
launch that forces the general one -- so that no comparison passes by both launches running the same code.  The plain launch
is forced into the general instantiation by requesting a hit-index AOV, which changes no pixel.  Frames are compared byte
for byte with each other, with the straightforward kernel (variant 1) and with the CPU oracle; ray and probe counters of the
counting launches (the STATS siblings of the same instantiations) with the oracle's."""
import numpy as np
import pytest

from tests import grid_shape_cases as gsc
from tests import helpers

pytestmark = pytest.mark.gpu

W, H = 64, 48
INV = helpers.INV
LIGHT = (INV, INV, INV)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import voxelengine_amd as vx
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ctx = helpers.new_ctx(vx)
    ctx.SetOrthoWindowSize(200.0, 200.0)
    yield vx, ctx, torch
    ctx.close()


def _scene_voxels():
    """256^3 (8 coarse cells an axis at brick edge 32): a bumpy floor, towers and a floating slab that cast shadows, a wall on
    the +x face and sparse single voxels everywhere, so that rays end inside bricks, between them and outside the grid"""
    rng = np.random.default_rng(32)
    v = np.zeros((256, 256, 256), bool)
    h = np.repeat(np.repeat(rng.integers(6, 30, size=(48, 48)), 4, 0), 4, 1)
    for y in range(30):
        v[32:224, 16 + y, 32:224] = h > y
    v[80:96, 16:170, 80:96] = True
    v[160:176, 16:120, 120:150] = True
    v[100:180, 140:148, 150:200] = True
    v[255, 0:100, :] = True
    n = 3000
    v[rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)] = True
    return v


@pytest.fixture(scope="module")
def worlds(vxo):
    """the same voxels at brick edge 32 (the COMMON instantiations' world), 16 and 8"""
    v = _scene_voxels()
    return {f: vxo.World.from_voxels(v, f) for f in (32, 16, 8)}


def _cam(pos, target):
    f = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, (0.0, 1.0, 0.0))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    as32 = lambda v: tuple(float(np.float32(c)) for c in v)
    return (as32(pos), as32(f), as32(u), as32(r))


# three different cameras inside the grid: above the terrain, among the towers, low and grazing
CAMS = [_cam((128.0, 200.0, 128.0), (120.0, 30.0, 110.0)), _cam((50.5, 120.0, 210.25), (128.0, 40.0, 128.0)),
        _cam((200.0, 60.0, 40.0), (100.0, 30.0, 150.0))]
FRAME_NUMBERS = [3, 8, 4]

_oracle_cache = {}


def _oracle(vxo, w, key, cams, okw, frame_numbers, width, height):
    """the oracle's frames of `cams` (fb, hit indices), and the sums of its ray and probe counters; computed once per key"""
    if key in _oracle_cache:
        return _oracle_cache[key]
    ckw = dict(mode=okw.get("mode", 0), checkerboard=int(okw.get("checkerboard", False)), shadow=int(okw.get("shadow", False)),
               bounce_samples=okw.get("bounce_samples", 0), bounce_all_hits=int(okw.get("bounce_all_hits", False)),
               ortho=int(okw.get("ortho", False)), bounce_depth=okw.get("bounce_depth", 1), ortho_size=(200.0, 200.0), light_dir=LIGHT)
    frames, rays, probes = [], np.zeros(4, np.int64), np.zeros(3, np.int64)
    for (pos, f, u, r), fn in zip(cams, frame_numbers):
        p = vxo.make_params(width, height, pos, f, u, r, frame_number=fn, **ckw)
        out = w.render(p, fb=np.zeros((height, width, 4), np.uint8), want_hit=True, nthreads=16)
        st = out["stats"]
        rays += (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits)
        probes += (st.probes.coarse_probes, st.probes.brick_entries, st.probes.fine_probes)
        for a in (out["fb"], out["hit"]):
            a.setflags(write=False)
        frames.append((out["fb"], out["hit"]))
    _oracle_cache[key] = (frames, rays, probes)
    return _oracle_cache[key]


def _launch(gpu, cams, okw, frame_numbers, *, variant=4, stats=False, multi=False, hit_views=(), color=False, width=W, height=H):
    """one launch (multi: RenderViews of all `cams`; else one RenderScreen per camera): frames, colour AOVs, hit indices, stats"""
    vx, ctx, torch = gpu
    ctx.set_kernel_variant(variant)
    try:
        fbs = [torch.zeros((height, width, 4), dtype=torch.uint8, device="cuda") for _ in cams]
        cols = [torch.full((height, width, 3), -3.0, dtype=torch.float32, device="cuda") if color else None for _ in cams]
        hits = [torch.full((height, width), -7, dtype=torch.int64, device="cuda") if k in hit_views else None for k in range(len(cams))]
        ctx.frame_stats()
        if multi:
            opts = vx.RenderOptions(collect_stats=stats, **okw)
            ctx.RenderViews(width, height, [dict(fb=fbs[k], origin=c[0], fwd=c[1], up=c[2], right=c[3], frame_number=frame_numbers[k],
                                                 color_aov=cols[k], hit_aov=hits[k]) for k, c in enumerate(cams)], opts)
        else:
            for k, c in enumerate(cams):
                opts = vx.RenderOptions(collect_stats=stats, frame_number=frame_numbers[k], **okw)
                ctx.RenderScreen(width, height, fbs[k], c[0], c[1], c[2], c[3], opts, color_aov=cols[k], hit_aov=hits[k])
        st = ctx.frame_stats()
        return ([f.cpu().numpy() for f in fbs], [None if c is None else c.cpu().numpy() for c in cols],
                [None if h is None else h.cpu().numpy() for h in hits], st)
    finally:
        ctx.set_kernel_variant(4)


def _specialisation(gpu, okw, nviews, width, height, hit_aov=None, accum=None):
    vx, ctx, torch = gpu
    return ctx.render_specialisation(width, height, vx.RenderOptions(**okw), nviews=nviews, hit_aov=hit_aov, accum=accum)


def _plain_against_general(gpu, vxo, w, key, cams, okw, *, multi, color=False, frame_numbers=None, width=W, height=H):
    """The plain launch (COMMON instantiation) and the same launch with a hit-index AOV (general instantiation), timed and
    counting, and variant 1, against the oracle.  Returns the oracle's ray counters."""
    vx, ctx, torch = gpu
    frame_numbers = frame_numbers or FRAME_NUMBERS[:len(cams)]
    nviews = len(cams) if multi else 0
    # a multi-view launch is general as soon as ONE view has the AOV; single-view launches each carry their own
    hit_views = (1,) if multi and len(cams) > 1 else tuple(range(len(cams)))
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert _specialisation(gpu, okw, nviews, width, height) == 1
    assert _specialisation(gpu, okw, nviews, width, height, hit_aov=probe) == 0
    ctx.set_kernel_variant(1)
    try:
        assert _specialisation(gpu, okw, nviews, width, height) == 0  # (variant 1 is another kernel altogether)
    finally:
        ctx.set_kernel_variant(4)
    want, rays, probes = _oracle(vxo, w, key, cams, okw, frame_numbers, width, height)
    kw = dict(multi=multi, color=color, width=width, height=height)
    plain = _launch(gpu, cams, okw, frame_numbers, **kw)
    general = _launch(gpu, cams, okw, frame_numbers, hit_views=hit_views, **kw)
    plain_s = _launch(gpu, cams, okw, frame_numbers, stats=True, **kw)
    general_s = _launch(gpu, cams, okw, frame_numbers, stats=True, hit_views=hit_views, **kw)
    direct = _launch(gpu, cams, okw, frame_numbers, variant=1, **kw)
    for tag, (fbs, cols, hits, st) in (("plain", plain), ("general", general), ("plain, counting", plain_s),
                                       ("general, counting", general_s), ("variant 1", direct)):
        for k in range(len(cams)):
            assert fbs[k].tobytes() == plain[0][k].tobytes(), (tag, k)
            assert np.array_equal(fbs[k], want[k][0]), (tag, k)
            if color and tag != "variant 1":
                assert cols[k].tobytes() == plain[1][k].tobytes(), (tag, k)
            if hits[k] is not None:
                assert np.array_equal(hits[k], want[k][1]), (tag, k)
        assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == tuple(int(v) for v in rays), tag
        if "counting" in tag:
            assert (st.coarse_probes, st.brick_entries, st.fine_probes) == tuple(int(v) for v in probes), tag
            assert st.guard_stray_loads == 0
    if color:
        for k in range(len(cams)):  # the AOV was written: no pixel of the fill value is left
            assert not np.any(plain[1][k] == -3.0)
    return rays


OPTIONS = {
    "primary only": dict(shadow=False, bounce_samples=0),
    "shadow": dict(shadow=True, bounce_samples=0),
    "one sample": dict(shadow=False, bounce_samples=1),
    "shadow, one sample": dict(shadow=True, bounce_samples=1),
    "shadow, three samples": dict(shadow=True, bounce_samples=3),
    "shadow, three samples, all hits": dict(shadow=True, bounce_samples=3, bounce_all_hits=True),
    "one sample, all hits": dict(shadow=False, bounce_samples=1, bounce_all_hits=True),
    "shadow, one sample, depth 2": dict(shadow=True, bounce_samples=1, bounce_depth=2),
    "shadow, three samples, all hits, depth 2": dict(shadow=True, bounce_samples=3, bounce_all_hits=True, bounce_depth=2),
    "three samples, all hits, depth 2": dict(shadow=False, bounce_samples=3, bounce_all_hits=True, bounce_depth=2),
}


@pytest.mark.parametrize("color", [False, True], ids=["", "colour AOV"])
@pytest.mark.parametrize("multi", [False, True], ids=["single view", "three views"])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_plain_frame_equals_the_general_instantiation(gpu, vxo, worlds, name, multi, color):
    w = worlds[32]
    helpers.upload(gpu[1], w)
    okw = OPTIONS[name]
    rays = _plain_against_general(gpu, vxo, w, ("matrix", name), CAMS, okw, multi=multi, color=color)
    # the options do what they say: primary hits everywhere, shadow rays and samples exactly when asked for
    assert rays[0] == 3 * W * H and rays[3] > W * H
    assert (rays[1] > 0) == okw["shadow"] and (rays[2] > 0) == (okw["bounce_samples"] > 0)


SHAPES = {
    "83 x 61": (83, 61, CAMS[:2]),
    "8 x 8": (8, 8, CAMS[:2]),
    "1 x 1": (1, 1, CAMS[:2]),
    "centre tile with the crosshair, 24 x 24": (24, 24, CAMS[:2]),
    "tall, 16 x 200": (16, 200, CAMS[:2]),
    "camera outside the grid": (W, H, [_cam((-60.0, 300.0, -40.0), (128.0, 40.0, 128.0)), _cam((330.0, 90.0, 128.0), (128.0, 60.0, 120.0))]),
    "top-down camera": (W, H, None),
}


@pytest.mark.parametrize("multi", [False, True], ids=["single view", "two views"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_frame_shapes_of_the_folded_pixel_map(gpu, vxo, worlds, name, multi):
    """Where liveness, the crosshair and the tile edges of the folded pixel_coords can go wrong."""
    vx, ctx, torch = gpu
    w = worlds[32]
    helpers.upload(ctx, w)
    width, height, cams = SHAPES[name]
    if cams is None:  # straight down from above the grid (helpers.CAMERAS["C"]), and from inside it
        f, u, r = vx.GetDirections((-1.5707, 0.0, 0.0))
        cams = [((128.0, 384.0, 128.0), f, u, r), ((120.5, 180.0, 133.25), f, u, r)]
    okw = dict(shadow=True, bounce_samples=1)
    rays = _plain_against_general(gpu, vxo, w, ("shape", name), cams, okw, multi=multi, color=True, width=width, height=height)
    assert rays[0] == len(cams) * width * height
    if "crosshair" in name or name == "8 x 8":  # the launch's centre pixel is the crosshair: white in every view
        fbs = _launch(gpu, cams, okw, FRAME_NUMBERS[:2], multi=multi, width=width, height=height)[0]
        for fb in fbs:
            assert tuple(fb[height // 2, width // 2]) == (255, 255, 255, 255)
    if name == "camera outside the grid":
        assert 0 < rays[3] < rays[0]  # rays enter through the world slab, and some miss


def _one_frame(gpu, vxo, w, key, okw, *, cam=CAMS[0], frame_number=3):
    """a launch that must NOT take the COMMON path: 0 from the query, and the oracle's frame from the timed and the counting launch"""
    assert _specialisation(gpu, okw, 0, W, H) == 0
    assert _specialisation(gpu, okw, 2, W, H) == 0
    want, rays, probes = _oracle(vxo, w, key, [cam], okw, [frame_number], W, H)
    for stats in (False, True):
        fbs, _, _, st = _launch(gpu, [cam], okw, [frame_number], stats=stats)
        assert np.array_equal(fbs[0], want[0][0]), stats
        assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == tuple(int(v) for v in rays)
    return rays


@pytest.mark.parametrize("name,okw", [
    ("debug view", dict(mode=1, shadow=True, bounce_samples=1)),
    ("orthographic", dict(ortho=True, shadow=True, bounce_samples=1)),
    ("checkerboard", dict(checkerboard=True, shadow=True, bounce_samples=1)),
])
def test_frame_flags_outside_the_common_path(gpu, vxo, worlds, name, okw):
    w = worlds[32]
    helpers.upload(gpu[1], w)
    rays = _one_frame(gpu, vxo, w, ("general", name), okw)
    assert rays[3] > 0


@pytest.mark.parametrize("factor", [8, 16])
def test_other_brick_edges_run_the_general_instantiation(gpu, vxo, worlds, factor):
    w = worlds[factor]
    helpers.upload(gpu[1], w)
    rays = _one_frame(gpu, vxo, w, ("brick", factor), dict(shadow=True, bounce_samples=1))
    assert rays[1] == rays[3] > 0


def test_wide_grid_of_brick_edge_32_runs_the_general_instantiation(gpu, vxo):
    """tests/grid_shape_cases.py W2_f32: the smallest grid wide by one disjunct alone (8 x 512 x 8 cells), at brick edge 32 --
    only the grid keeps it off the COMMON path."""
    vx, ctx, torch = gpu
    case = gsc.BY_NAME["W2_f32"]
    w = gsc.world(vxo, case)
    assert w.factor == 32 and gsc.wide_disjuncts(case.cells, gsc.read_caps())
    helpers.upload(ctx, w)
    view = gsc.views(case)[0]
    ctx.SetFOV(gsc.VIEW_FOV)
    try:
        okw = dict(shadow=True, bounce_samples=1)
        assert _specialisation(gpu, okw, 0, W, H) == 0 and _specialisation(gpu, okw, 3, W, H) == 0
        pos, f, u, r = view["cam"]
        p = vxo.make_params(W, H, pos, f, u, r, frame_number=3, shadow=1, bounce_samples=1, light_dir=LIGHT, **view["kw"])
        want = w.render(p, fb=np.zeros((H, W, 4), np.uint8), nthreads=16)
        for stats in (False, True):
            fbs, _, _, st = _launch(gpu, [view["cam"]], okw, [3], stats=stats)
            assert np.array_equal(fbs[0], want["fb"]), stats
            assert st.primary_hits == want["stats"].primary_hits > 0
    finally:
        ctx.SetFOV(90.0)


@pytest.mark.parametrize("compact", [False, True], ids=["frame rows", "packed rows"])
def test_two_strips_run_the_general_instantiation(gpu, vxo, worlds, compact):
    """strip_count = 2: each shard renders its own rows, into the frame itself or into a packed buffer of its own; together
    they are the oracle's frame"""
    vx, ctx, torch = gpu
    w = worlds[32]
    helpers.upload(ctx, w)
    okw = dict(shadow=True, bounce_samples=1)
    pos, f, u, r = CAMS[0]
    want, rays, _ = _oracle(vxo, w, ("matrix", "shadow, one sample", 0), [CAMS[0]], okw, [3], W, H)
    rows, count = 8, 2
    max_rows = max(vx.compact_rows(H, rows, count, i) for i in range(count))
    stride = max_rows * W * 4
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    shards = torch.zeros((count, stride), dtype=torch.uint8, device="cuda")
    ctx.frame_stats()
    for i in range(count):
        skw = dict(strip_rows=rows, strip_count=count, strip_index=i, compact=compact, **okw)
        assert _specialisation(gpu, skw, 0, W, H) == 0
        ctx.RenderScreen(W, H, shards[i] if compact else out, pos, f, u, r, vx.RenderOptions(frame_number=3, **skw))
    st = ctx.frame_stats()
    if compact:
        ctx.deinterleave_strips(W, H, rows, count, shards, stride, out)
    assert np.array_equal(out.cpu().numpy(), want[0][0])
    assert (st.primary_rays, st.shadow_rays, st.bounce_rays, st.primary_hits) == tuple(int(v) for v in rays)


def test_accumulation_runs_the_general_instantiation(gpu, vxo, worlds):
    vx, ctx, torch = gpu
    w = worlds[32]
    helpers.upload(ctx, w)
    okw = dict(shadow=True, bounce_samples=1)
    pos, f, u, r = CAMS[0]
    acc_c, fb_c = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.uint8)
    acc_g = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    fb_g = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    assert _specialisation(gpu, okw, 0, W, H) == 1 and _specialisation(gpu, okw, 0, W, H, accum=acc_g) == 0
    for frame in (1, 2, 3):
        p = vxo.make_params(W, H, pos, f, u, r, frame_number=frame, shadow=1, bounce_samples=1, light_dir=LIGHT)
        w.render(p, fb=fb_c, accum=acc_c, accum_reset=frame == 3, nthreads=16)
        ctx.RenderScreen(W, H, fb_g, pos, f, u, r, vx.RenderOptions(frame_number=frame, **okw), accum=acc_g, accum_reset=frame == 3)
        assert np.array_equal(fb_g.cpu().numpy(), fb_c), frame
        assert np.array_equal(acc_g.cpu().numpy().view(np.uint32), acc_c.view(np.uint32)), frame
