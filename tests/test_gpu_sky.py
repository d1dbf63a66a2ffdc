"""The sky on frames on the device (include/vxrt.h, vxrt_sky_frame): colours, the BGRA8 frame and the summary bit-equal to
tests/ref_sky.py on the random cases of the host tests -- frames that straddle a wave's 64 lanes and a workgroup's 4 rows,
both launch shapes, with and without clouds, every glow exponent, one and six octaves, both cameras, in place and out of
place, guard bytes behind every buffer --; the hand-derived cases; the whole path on rendered frames (render with AOVs,
guides, sky) under six views and behind the material and light stages; the frame limits; a side stream, a captured graph
replayed three times; every refusal in the documented order with nothing written; and the headless example's sky line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import ref_denoise as R
from tests import ref_sky as SK
from tests import sky_cases as SC
from tests.helpers import eng, gen_dense, new_ctx, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GUARD_BYTES = 256
W, H = 96, 64
ORTHO_SIZE = (40.0, 30.0)
_CACHE = {}


def _case(Wf, Hf, ortho, pose):
    key = (Wf, Hf, ortho, pose)
    if key not in _CACHE:
        case = SC.random_case(Wf, Hf, ortho, pose)
        _CACHE[key] = (case, {s: SC.run_case(case, SC.PARAM_SETS[s])[:2] for s in range(len(SC.PARAM_SETS))})
    return _CACHE[key]


def _guarded(torch, a=None, nbytes=0, fill=0x7B):
    """a device byte tensor holding the numpy array `a` (or `nbytes` bytes of `fill`) with GUARD_BYTES bytes of 0x5A behind it"""
    raw = np.full(nbytes, fill, np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.full((raw.size + GUARD_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    t[:raw.size].copy_(torch.from_numpy(raw.copy()))
    return t


def _payload(t, dtype, shape):
    return t[:-GUARD_BYTES].cpu().numpy().view(dtype).reshape(shape)


def _sky(vx, case, p=None):
    return vx.Sky(**dict(SK.DAY, **dict(case["params"], **(p or {}))))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def bare(eng):
    """a context without a world: the stage needs none"""
    vx, _ = eng
    c = new_ctx(vx)
    yield c
    c.close()


# ---- bit-equality on small frames --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wf,Hf,ortho,pose", SC.CASES)
def test_the_device_equals_the_restatement(eng, bare, Wf, Hf, ortho, pose):
    """through the C ABI, every buffer with guard bytes behind it: every parameter set with every output (the counting launch);
    without framebuffer and summary (the plain launch) -- the same pixels --; the colour output aliasing the input"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    case, wants = _case(Wf, Hf, ortho, pose)
    n = Wf * Hf
    bare.SetOrthoWindowSize(*case["ortho_size"])
    modes = [(s, "all") for s in range(len(SC.PARAM_SETS))] + [(s, "bare") for s in (1, 9)] + [(1, "alias"), (1, "alias bare")]
    for s, mode in modes:
        color, summary = wants[s]
        d_col, d_keys = _guarded(torch, case["color"]), _guarded(torch, case["keys"])
        d_out, d_fb, d_sum = _guarded(torch, nbytes=12 * n), _guarded(torch, nbytes=4 * n), _guarded(torch, nbytes=24)
        plain = mode.endswith("bare")
        out = d_col if mode.startswith("alias") else d_out
        p = _sky(vx, case, SC.PARAM_SETS[s])._c(case["cam"], ortho)
        rc = L.vxrt_sky_frame(bare._h, Wf, Hf, d_col.data_ptr(), d_keys.data_ptr(), C.byref(p), out.data_ptr(),
                              None if plain else d_fb.data_ptr(), None if plain else d_sum.data_ptr(), None)
        assert rc == 0, L.vxrt_last_error()
        torch.cuda.synchronize()
        what = (Wf, Hf, ortho, pose, s, mode)
        assert np.array_equal(R.bits(_payload(out, F32, (Hf, Wf, 3))), R.bits(color)), what
        if plain:
            for t in (d_fb, d_sum):
                assert bool((t[:-GUARD_BYTES] == 0x7B).all()), what
        else:
            assert np.array_equal(_payload(d_fb, np.uint8, (Hf, Wf, 4)), R.bgra8(color)), what
            assert tuple(_payload(d_sum, np.uint32, (6,)).tolist()) == summary, what
        for t in (d_col, d_keys, d_out, d_fb, d_sum):
            assert bool((t[-GUARD_BYTES:] == 0x5A).all()), what
        assert np.array_equal(_payload(d_keys, np.uint32, (Hf, Wf)), case["keys"]), what
        if mode.startswith("alias"):
            assert bool((d_out[:-GUARD_BYTES] == 0x7B).all()), what
        else:
            assert np.array_equal(R.bits(_payload(d_col, F32, (Hf, Wf, 3))), R.bits(case["color"])), what


def test_the_hand_derived_cases_on_the_device(eng, bare):
    vx, torch = eng
    bare.SetOrthoWindowSize(*SC.WINDOW)
    for index, make in enumerate(SC.HAND_CASES):
        case, color, summary = make()
        got = bare.sky_frame(_dev(torch, case["color"]), _dev(torch, case["keys"].view(np.int32)), case["cam"], _sky(vx, case), ortho=True, summary=True)
        assert np.array_equal(R.bits(got.color.cpu().numpy()[0, 0]), R.bits(np.asarray(color, F32))), (index, got.color)
        assert tuple(got.summary) == summary, index
    case = SC.ortho_frame()
    bare.SetOrthoWindowSize(*case["ortho_size"])
    got = bare.sky_frame(_dev(torch, case["color"]), _dev(torch, case["keys"].view(np.int32)), case["cam"], _sky(vx, case), ortho=True, summary=True)
    assert bool((got.color == torch.tensor([1.0, 0.5, 0.25], device="cuda")).all()) and tuple(got.summary) == (64, 0, 0, 64, 0, 0)


def test_a_frame_on_which_the_counting_launch_walks_several_tiles_per_wave(eng, bare):
    """with a summary the launch is at most two workgroups of 16 waves per compute unit: 1990 x 262 is 2112 tiles of 64 x 4,
    more than the 2048 groups of four waves a device of 256 compute units gets, and neither side is a multiple of the tile;
    the same frame without a summary (one tile per workgroup) gives the same bits.  Through the Python mirror."""
    vx, torch = eng
    Wf, Hf = 1990, 262
    case = SC.random_case(Wf, Hf, False, "level")
    color, summary, _ = SC.run_case(case, SC.PARAM_SETS[3])
    bare.SetOrthoWindowSize(*case["ortho_size"])
    args = (_dev(torch, case["color"]), _dev(torch, case["keys"].view(np.int32)), case["cam"], _sky(vx, case, SC.PARAM_SETS[3]))
    counted = bare.sky_frame(*args, summary=True)
    plain = bare.sky_frame(*args)  # (the default: no summary)
    torch.cuda.synchronize()
    assert tuple(counted.summary) == summary and min(summary) > 1000 and plain.summary is None
    for got in (counted, plain):
        assert np.array_equal(R.bits(got.color.cpu().numpy()), R.bits(color))


# ---- the whole path on rendered frames ---------------------------------------------------------------------------------
DIMS = (128, 128, 128)
UP = ((64.0, 126.0, 64.0), (0.1, 0.98, 0.15), (0.0, -0.15, 0.98), (1.0, 0.0, -0.1))
SKY = dict(SK.DAY, flags=SK.CLOUDS, cloud_y=200.0, cloud_scale=0.03, fog_start=8.0, fog_density=0.02, cos_inner=0.99, cos_outer=0.95)


@pytest.fixture(scope="module")
def scene(eng, vxo):
    vx, _ = eng
    w = vxo.World.generate(vxo.GEN_INT_TERRAIN, *DIMS, 16)
    c = new_ctx(vx)
    c.SetOrthoWindowSize(*ORTHO_SIZE)
    upload(c, w)
    yield c, w
    c.close()


def _render(vx, torch, ctx, cam, ortho, stream=None):
    pos, f, u, r = cam
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.full((H, W), -7, dtype=torch.int64, device="cuda")
    opts = vx.RenderOptions(shadow=True, bounce_samples=1, bounce_all_hits=True, ortho=ortho, frame_number=3)
    ctx.RenderScreen(W, H, fb, pos, f, u, r, opts, color_aov=col, hit_aov=hit, stream=stream)
    keys = ctx.frame_guides(W, H, pos, f, u, r, hit, ortho=ortho, stream=stream)
    return fb, col, hit, keys


def _want(col, keys, cam, ortho, p):
    return SK.sky_frame(col.cpu().numpy(), keys.cpu().numpy().view(np.uint32), cam, p, ortho, ortho_size=ORTHO_SIZE)


def _assert_sky(got, fb, want, what):
    assert np.array_equal(R.bits(got.color.cpu().numpy()), R.bits(want[0])), what
    assert np.array_equal(fb.cpu().numpy(), R.bgra8(want[0])), what
    assert tuple(got.summary) == want[1], what


VIEWS = {  # camera, ortho, parameters
    "up": (UP, False, SKY),
    "down": ("C", False, SKY),
    "ground": ("D", False, SKY),
    "slant": ("A", False, SKY),
    "above": ("A", False, dict(SKY, cloud_y=50.0)),
    "ortho": ("A", True, SKY),
}


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_render_guides_sky_equals_the_restatement(eng, vxo, scene, view):
    """the restatement applied to the colour AOV and the keys the device made (the render and the guides have tests of their
    own): a camera looking up sees sky alone, one looking down from above ground and fogged terrain, one on the ground all of it"""
    vx, torch = eng
    ctx, w = scene
    cam, ortho, p = VIEWS[view]
    cam = helpers.camera(cam, DIMS, vxo) if isinstance(cam, str) else cam
    fb, col, hit, keys = _render(vx, torch, ctx, cam, ortho)
    got = ctx.sky_frame(col, keys, cam, vx.Sky(**p), ortho=ortho, fb=fb, summary=True)
    torch.cuda.synchronize()
    want = _want(col, keys, cam, ortho, p)
    _assert_sky(got, fb, want, view)
    miss, hitn, ground, sun, cloud, fogged = want[1]
    print("sky pipeline", view, "miss, hit, ground, sun, cloud, fogged", want[1])
    assert miss + hitn == W * H
    if view == "up":  # above the terrain, looking up: sky alone
        assert miss == W * H and ground == 0
    if view == "down":  # 192 voxels above a world 128 wide under a 90 degree lens: terrain in the middle, ground colour around it,
        assert hitn > 0 and ground > 0 and fogged == hitn and cloud == 0  # and every hit farther than fog_start
    if view == "above":
        assert cloud == 0


def test_behind_the_material_and_light_stages_without_fog_no_hit_pixel_changes(eng, vxo, scene):
    vx, torch = eng
    ctx, w = scene
    cam = helpers.camera("A", DIMS, vxo)
    fb, col, hit, keys = _render(vx, torch, ctx, cam, False)
    rules = vx.MaterialRules(((None, 1, 2, 3, 3),))
    mat = ctx.material_frame(col, keys, hit, cam, rules, vx.Palette().set(1, (0.4, 0.8, 0.3)).set(2, (0.5, 0.4, 0.3)))
    lit = ctx.light_frame(mat.color, keys, hit, cam)
    p = dict(SKY, fog_density=0.0)
    got = ctx.sky_frame(lit.color, keys, cam, vx.Sky(**p), fb=fb, summary=True)
    torch.cuda.synchronize()
    _assert_sky(got, fb, _want(lit.color, keys, cam, False, p), "stages")
    hits = (keys != 0).cpu().numpy()
    before, after = lit.color.cpu().numpy(), got.color.cpu().numpy()
    assert np.array_equal(R.bits(before[hits]), R.bits(after[hits])) and hits.sum() > 0 and got.summary.fogged == 0
    assert (~hits).sum() == 0 or not np.array_equal(R.bits(before[~hits]), R.bits(after[~hits]))


# ---- the frame limits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wf,Hf", ((65535, 1), (1, 65535)))
def test_the_longest_row_and_the_longest_column(eng, bare, Wf, Hf):
    vx, torch = eng
    case = SC.random_case(Wf, Hf, False, "level")
    color, summary, _ = SC.run_case(case, SC.PARAM_SETS[3])
    bare.SetOrthoWindowSize(*case["ortho_size"])
    fb = torch.zeros((Hf, Wf, 4), dtype=torch.uint8, device="cuda")
    got = bare.sky_frame(_dev(torch, case["color"]), _dev(torch, case["keys"].view(np.int32)), case["cam"], _sky(vx, case, SC.PARAM_SETS[3]), fb=fb, summary=True)
    plain = bare.sky_frame(_dev(torch, case["color"]), _dev(torch, case["keys"].view(np.int32)), case["cam"], _sky(vx, case, SC.PARAM_SETS[3]),
                           summary=False)
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(got.color.cpu().numpy()), R.bits(color)) and tuple(got.summary) == summary
    assert np.array_equal(R.bits(plain.color.cpu().numpy()), R.bits(color)) and np.array_equal(fb.cpu().numpy(), R.bgra8(color))


def test_the_largest_frame_on_a_sample_of_pixels(eng, bare):
    """8192 x 8192 = 2^26 pixels: the first and the last row and 2^16 seeded pixels (512 rows, 128 pixels of each) against the
    vectorised restatement evaluated on those pixels; the keys and colours are functions of the pixel index made on the
    device (the colours are read back at the sample).  One pixel more on either side is refused."""
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    Wf = Hf = 8192
    n = Wf * Hf
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    r = (idx * 2654435761) & 0xFFFFFFFF
    # a third of the pixels miss; the others show a face of axis 0 .. 2 at plane 0 .. 4095
    keys64 = torch.where(r % 3 == 0, torch.zeros_like(r), (1 << 31) | (((r >> 8) % 3) << 26) | (((r >> 4) & 1) << 25) | ((r >> 12) & 4095))
    keys = (keys64 - ((keys64 >> 31) << 32)).to(torch.int32)  # (the same 32 bits as an int32)
    del keys64, r
    color = ((idx % 1021).to(torch.float32) / 1021.0).view(Hf, Wf, 1).expand(Hf, Wf, 3).contiguous()
    del idx
    cam = tuple(np.asarray(v, F32) for v in SC.POSES["level"])
    p = dict(SC.random_params(np.random.default_rng(3), "level"), flags=SK.CLOUDS, glow_log2=4, octaves=6)
    bare.SetOrthoWindowSize(*SC.ORTHO_SIZE)
    got = bare.sky_frame(color, keys, cam, vx.Sky(**dict(SK.DAY, **p)), summary=True)
    torch.cuda.synchronize()
    rng = np.random.default_rng(11)
    rows = rng.choice(Hf, 512, replace=False)
    pixels = np.concatenate([np.stack([rng.integers(0, Wf, 128), np.full(128, y)], -1) for y in rows] +
                            [np.stack([np.arange(Wf), np.full(Wf, y)], -1) for y in (0, Hf - 1)])
    at = pixels[:, 1] * Wf + pixels[:, 0]
    k = (at * 2654435761) & 0xFFFFFFFF
    want_keys = np.where(k % 3 == 0, 0, (1 << 31) | (((k >> 8) % 3) << 26) | (((k >> 4) & 1) << 25) | ((k >> 12) & 4095)).astype(np.uint32)
    sel = torch.from_numpy(at).cuda()
    assert np.array_equal(keys.view(-1)[sel].cpu().numpy().view(np.uint32), want_keys)
    want = SK.sky_frame(color.view(-1, 3)[sel].cpu().numpy(), want_keys, cam, p, ortho_size=SC.ORTHO_SIZE, pixels=pixels, dims=(Wf, Hf))
    assert np.array_equal(R.bits(got.color.view(-1, 3)[sel].cpu().numpy()), R.bits(want[0]))
    s = got.summary
    assert s.miss + s.hit == n and s.miss == int((keys == 0).sum()) and min(want[1]) > 0 and s.cloud > want[1][4] and s.fogged > want[1][5]
    sp = vx.Sky()._c(cam)
    for Wb, Hb in ((8193, 8192), (8192, 8193), (65536, 1), (1, 65536), (0, 1)):
        assert L.vxrt_sky_frame(bare._h, Wb, Hb, color.data_ptr(), keys.data_ptr(), C.byref(sp), color.data_ptr(), None, None, None) == -1
        assert "W, H" in L.vxrt_last_error().decode()


# ---- call rules --------------------------------------------------------------------------------------------------------
def test_the_same_on_a_side_stream(eng, vxo, scene):
    vx, torch = eng
    ctx, w = scene
    cam = helpers.camera("D", DIMS, vxo)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        fb, col, hit, keys = _render(vx, torch, ctx, cam, False, stream=side.cuda_stream)
        got = ctx.sky_frame(col, keys, cam, vx.Sky(**SKY), fb=fb, summary=True, stream=side.cuda_stream)
    side.synchronize()
    _assert_sky(got, fb, _want(col, keys, cam, False, SKY), "side stream")


def test_capture_and_three_replays_equal_the_eager_call(eng, vxo, scene):
    """vxrt_sky_frame captured on a side stream and replayed three times into poisoned outputs"""
    vx, torch = eng
    ctx, w = scene
    cam = helpers.camera("D", DIMS, vxo)
    fb, col, hit, keys = _render(vx, torch, ctx, cam, False)
    eager = ctx.sky_frame(col, keys, cam, vx.Sky(**SKY), fb=fb, summary=True)
    torch.cuda.synchronize()
    _assert_sky(eager, fb, _want(col, keys, cam, False, SKY), "eager")
    side = torch.cuda.Stream()
    out, fb2 = torch.zeros_like(col), torch.zeros_like(fb)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        res = ctx.sky_frame(col, keys, cam, vx.Sky(**SKY), out=out, fb=fb2, summary=True)
    assert not out.any() and not fb2.any()  # capturing ran nothing
    for _ in range(3):
        with torch.cuda.stream(side):  # (the poison on the replay's stream: ordered before it)
            out.fill_(7.0)
            fb2.fill_(9)
            res._summary.fill_(77)
            g.replay()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.color.view(torch.int32)) and torch.equal(fb2, fb)
        assert tuple(int(v) for v in res._summary.cpu()) == tuple(eager.summary)


def test_refusals_in_the_documented_order_with_nothing_written(eng, bare):
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    n = 16 * 8
    col = torch.full((8, 16, 3), 0.5, dtype=torch.float32, device="cuda")
    keys = torch.full((n,), 0, dtype=torch.int32, device="cuda")
    out = torch.full((8, 16, 3), 9.0, dtype=torch.float32, device="cuda")
    fb = torch.full((n,), 0x1234, dtype=torch.int32, device="cuda")
    summary = torch.full((6,), 0x1234, dtype=torch.int32, device="cuda")
    nan, inf = float("nan"), float("inf")

    def err():
        return L.vxrt_last_error().decode()

    def call(h=bare._h, Wf=16, Hf=8, size=208, params=True, reserved=0, bad=None, cp=col.data_ptr(), kp=keys.data_ptr(), op=out.data_ptr(), **sky):
        p = vx.Sky(**sky)._c(((1, 2, 3), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
        p.struct_size, p.reserved_ = size, reserved
        if bad:
            field, k, v = bad
            getattr(p.cam, field)[k] = v
        return L.vxrt_sky_frame(h, Wf, Hf, cp, kp, C.byref(p) if params else None, op, fb.data_ptr(), summary.data_ptr(), None)

    # each call has the earlier faults mended and all the later ones still in it
    later = dict(size=8, flags=2, ground=(0.1, -1.0, 0.1), octaves=7, fog_start=nan, fog_max=1.5, cos_outer=1.0, sun_dir=(0.0, 0.0, 0.0),
                 bad=("fwd", 1, nan), cp=None)
    assert call(h=None, Wf=0, **later) == -1 and "ctx" in err()
    for Wf, Hf in ((0, 8), (16, 0), (65536, 1), (1, 65536), (8193, 8192)):
        assert call(Wf=Wf, Hf=Hf, **later) == -1 and "W, H" in err()
    assert call(**later) == -1 and "size" in err()
    later.pop("size")
    assert call(params=False, cp=None) == -1 and "size" in err()
    for flags in (2, 3, 1 << 31):
        assert call(**dict(later, flags=flags)) == -1 and "flags" in err()
    later.pop("flags")
    assert call(reserved=1, **later) == -1 and "flags" in err()
    for kw in (dict(ground=(0.1, -1.0, 0.1)), dict(zenith=(nan, 0.1, 0.1)), dict(horizon=(0.1, 0.1, inf)), dict(sun_color=(-0.5, 1.0, 1.0)),
               dict(cloud_color=(1.0, nan, 1.0))):
        assert call(**dict(later, **kw)) == -1 and "colour" in err()
    later.pop("ground")
    for kw in (dict(octaves=7), dict(octaves=0), dict(octaves=1, glow_log2=9)):
        assert call(**dict(later, **kw)) == -1 and "glow_log2" in err()
    later.pop("octaves")
    for kw in (dict(fog_start=nan), dict(fog_start=0.0, fog_density=-1.0), dict(fog_start=0.0, cloud_scale=inf), dict(fog_start=0.0, cloud_y=nan),
               dict(fog_start=0.0, cloud_offset=(0.0, inf)), dict(fog_start=0.0, glow_strength=-0.0001)):
        assert call(**dict(later, **kw)) == -1 and "scalar" in err()
    later.pop("fog_start")
    for kw in (dict(fog_max=1.5), dict(fog_max=1.0, cloud_cover=1.25)):
        assert call(**dict(later, **kw)) == -1 and "0 .. 1" in err()
    later.pop("fog_max")
    for kw in (dict(cos_outer=1.0), dict(cos_inner=0.5, cos_outer=0.5), dict(cos_inner=1.5, cos_outer=0.5), dict(cos_inner=0.5, cos_outer=-1.5),
               dict(cos_inner=nan, cos_outer=0.5)):
        assert call(**dict(later, **kw)) == -1 and "cos_outer" in err()
    later.pop("cos_outer")
    for sun in ((0.0, 0.0, 0.0), (nan, 1.0, 0.0), (0.0, inf, 0.0), (1e-30, 0.0, 0.0), (3e19, 0.0, 0.0)):
        assert call(**dict(later, sun_dir=sun)) == -1 and "sun_dir" in err()
    later.pop("sun_dir")
    for field in ("origin", "fwd", "up", "right"):
        for k, v in ((0, nan), (2, inf), (1, -inf)):
            assert call(**dict(later, bad=(field, k, v))) == -1 and "non-finite" in err()
    later.pop("bad")
    for kw in (dict(cp=None), dict(kp=None), dict(op=None)):
        assert call(**kw) == -1 and "NULL" in err()
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and bool((fb == 0x1234).all()) and bool((summary == 0x1234).all()) and bool((col == 0.5).all())
    # and the same arguments mended are accepted on a context without a world: every pixel a miss, every output written
    assert call() == 0
    torch.cuda.synchronize()
    assert summary.tolist()[:2] == [n, 0] and not bool((out == 9.0).any()) and not bool((fb == 0x1234).any())


def test_strided_tensors_are_refused_and_left_unchanged(eng, bare):
    vx, torch = eng
    Wf, Hf = 16, 8
    n = Wf * Hf
    cam = ((1.0, 2.0, 3.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    col = torch.full((Hf, Wf, 3), 0.5, dtype=torch.float32, device="cuda")
    keys = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    out = torch.full((Hf, Wf, 6), 9.0, dtype=torch.float32, device="cuda")
    fb = torch.full((2 * n,), 0x1234, dtype=torch.int32, device="cuda")
    for kw in (dict(out=out[:, :, ::2]), dict(fb=fb[::2]), dict(out=out.double()[:, :, :3].contiguous())):
        with pytest.raises(ValueError):
            bare.sky_frame(col, keys[:n], cam, **kw)
    with pytest.raises(ValueError):
        bare.sky_frame(col, keys[::2], cam)
    with pytest.raises(ValueError):
        bare.sky_frame(col[:, ::2], keys[:n // 2], cam)
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and bool((fb == 0x1234).all())


# ---- the example ---------------------------------------------------------------------------------------------------------
def test_headless_example_sky_line(eng, vxo, tmp_path):
    """examples/voxelapp_headless on a path of three poses with "0 sky clouds", "1 sky" and "2 sky off": the summary lines of
    frames 0 and 1 are those of the Python path on the same world with the example's preset, the dumped PPMs the finished
    frames, and frame 2 is the plain frame"""
    vx, torch = eng
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge, Wf, Hf = 256, 64, 48
    f32 = lambda v: tuple(float(F32(x)) for x in v)  # binary32 values: their repr reads back as the same binary32
    eulers = [f32((-0.25 + 0.3 * j, 0.7 + 0.01 * j, 0.0)) for j in range(3)]
    positions = [f32((edge * 0.25 + 0.5 * j, edge * 0.9 - 0.25 * j, edge * 0.25 + 0.25 * j)) for j in range(3)]
    (tmp_path / "path.txt").write_text("".join("%r %r %r %r %r %r\n" % (*p, *e) for p, e in zip(positions, eulers)))
    (tmp_path / "script.txt").write_text("0 sky clouds\n1 sky\n2 sky off\n")
    out = subprocess.run([exe, str(edge), "3", str(tmp_path / "sk"), str(Wf), str(Hf), "2", str(tmp_path / "path.txt"), "1", "1", "1",
                          "0x0x0", str(tmp_path / "script.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [x for x in out.stdout.splitlines() if x.startswith("sky ")]
    assert len(lines) == 2, out.stdout

    dense = gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(dense, edge, edge, edge, 32))
        seen = []
        for j in range(3):
            f, u, r = vxo.get_directions(eulers[j])
            cam = (positions[j], f, u, r)
            fb = torch.zeros((Hf, Wf, 4), dtype=torch.uint8, device="cuda")
            col = torch.zeros((Hf, Wf, 3), dtype=torch.float32, device="cuda")
            hit = torch.zeros((Hf, Wf), dtype=torch.int64, device="cuda")
            ctx.RenderScreen(Wf, Hf, fb, *cam, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=j), color_aov=col, hit_aov=hit)
            if j < 2:
                keys = ctx.frame_guides(Wf, Hf, *cam, hit)
                sky = vx.Sky(flags=vx.SKY_CLOUDS if j == 0 else 0, sun_dir=(helpers.INV,) * 3, cloud_y=2.0 * edge)
                s = ctx.sky_frame(col, keys, cam, sky, fb=fb, summary=True).summary
                assert lines[j] == "sky frame %d miss %d ground %d sun %d cloud %d fogged %d" % (j, s.miss, s.ground, s.sun, s.cloud, s.fogged), (j, lines)
                seen.append(s)
            torch.cuda.synchronize()
            ppm = open(tmp_path / ("sk_%04d.ppm" % j), "rb").read()
            rgb = np.frombuffer(ppm[-Wf * Hf * 3:], np.uint8).reshape(Hf, Wf, 3)
            assert np.array_equal(rgb, fb.cpu().numpy()[..., 2::-1]), j
        assert seen[0].miss + seen[0].hit == Wf * Hf and seen[1].cloud == 0
    finally:
        ctx.close()
