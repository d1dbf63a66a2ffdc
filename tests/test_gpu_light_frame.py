"""The light on frames on the device (include/vxrt.h, vxrt_light_frame): colours, the BGRA8 frame, the terms and the summary
bit-equal to tests/ref_light_frame.py on the random cases of the host tests under all four flag combinations, the colour
output aliasing the input, without framebuffer, terms and summary, without levels, guard bytes behind every input and output;
the whole path -- render with both AOVs, guides, the light field of a box with two emitters, the light on the frame --
bit-equal to the restatement applied to the oracle's frame and to tests/ref_light.py's field at every brick edge, again after
an edit that opens a roof and a relight; on a side stream and from a captured graph; every refusal in the documented order
with nothing written; and the headless example's lit line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import vxo_edit
from tests import helpers
from tests import light_frame_cases as LC
from tests import ref_denoise as R
from tests import ref_light
from tests import ref_light_frame as LF
from tests.helpers import eng, gen_dense, new_ctx, upload
from tests.test_gpu_denoise import WORLDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GUARD_BYTES = 256
BOTH = LF.SMOOTH | LF.OCCLUSION
W, H = 160, 96
SHADED = dict(shadow=1, bounce_samples=1, bounce_all_hits=1)
_CACHE = {}


def _case(Wf, Hf, ortho, pose):
    key = (Wf, Hf, ortho, pose)
    if key not in _CACHE:
        case = LC.random_case(Wf, Hf, ortho, pose)
        want = {(flags, True): LC.run_case(case, flags)[:3] for flags in LC.FLAG_SETS}
        want[BOTH, False] = LC.run_case(case, BOTH, levels=False)[:3]
        _CACHE[key] = (case, want)
    return _CACHE[key]


def _guarded(torch, a=None, nbytes=0, fill=0x7B):
    """a device byte tensor holding the numpy array `a` (or `nbytes` bytes of `fill`) with GUARD_BYTES bytes of 0x5A behind it"""
    raw = np.full(nbytes, fill, np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.full((raw.size + GUARD_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    t[:raw.size].copy_(torch.from_numpy(raw.copy()))
    return t


def _payload(t, dtype, shape):
    return t[:-GUARD_BYTES].cpu().numpy().view(dtype).reshape(shape)


def _params(N, case, flags, cam=None):
    p = case["params"]
    q = N.LightFrameParams(struct_size=C.sizeof(N.LightFrameParams), ortho=int(case["ortho"]), flags=flags, outside_level=p["outside_level"],
                           sky_floor=p["sky_floor"])
    q.block_color = (C.c_float * 3)(*p["block_color"])
    q.ao_curve = (C.c_float * 4)(*p["ao_curve"])
    q.cam.origin, q.cam.fwd, q.cam.up, q.cam.right = ((C.c_float * 3)(*[float(x) for x in v]) for v in (cam or case["cam"]))
    q.box_origin, q.box_dims = (C.c_int32 * 3)(*case["box"][0]), (C.c_int32 * 3)(*case["box"][1])
    return q


@pytest.mark.parametrize("Wf,Hf,ortho,pose", LC.CASES)
def test_the_device_equals_the_restatement(eng, vxo, Wf, Hf, ortho, pose):
    """through the C ABI, every buffer with guard bytes behind it: the four flag combinations with every output; the colour
    output aliasing the input; no framebuffer, terms or summary; no levels"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    case, wants = _case(Wf, Hf, ortho, pose)
    n = Wf * Hf
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(case["world"], 8))
        ctx.SetOrthoWindowSize(*case["ortho_size"])
        modes = [(flags, "all") for flags in LC.FLAG_SETS] + [(BOTH, "alias"), (BOTH, "bare"), (BOTH, "no levels")]
        for flags, mode in modes:
            color, terms, summary = wants[flags, mode != "no levels"]
            d_col, d_keys, d_hit = _guarded(torch, case["color"]), _guarded(torch, case["keys"]), _guarded(torch, case["hit"])
            d_lev = _guarded(torch, case["levels"].transpose(2, 1, 0))
            d_out, d_fb, d_terms = _guarded(torch, nbytes=12 * n), _guarded(torch, nbytes=4 * n), _guarded(torch, nbytes=12 * n)
            d_sum = _guarded(torch, nbytes=16)
            bare = mode == "bare"
            out = d_col if mode == "alias" else d_out
            rc = L.vxrt_light_frame(ctx._h, Wf, Hf, d_col.data_ptr(), d_keys.data_ptr(), d_hit.data_ptr(),
                                    None if mode == "no levels" else d_lev.data_ptr(), C.byref(_params(N, case, flags)), out.data_ptr(),
                                    None if bare else d_fb.data_ptr(), None if bare else d_terms.data_ptr(),
                                    None if bare else d_sum.data_ptr(), None)
            assert rc == 0, L.vxrt_last_error()
            torch.cuda.synchronize()
            what = (Wf, Hf, ortho, pose, flags, mode)
            assert np.array_equal(R.bits(_payload(out, F32, (Hf, Wf, 3))), R.bits(color)), what
            if bare:
                for t in (d_fb, d_terms, d_sum):
                    assert bool((t[:-GUARD_BYTES] == 0x7B).all()), what
            else:
                assert np.array_equal(_payload(d_fb, np.uint8, (Hf, Wf, 4)), R.bgra8(color)), what
                assert np.array_equal(R.bits(_payload(d_terms, F32, (Hf, Wf, 3))), R.bits(terms)), what
                assert tuple(_payload(d_sum, np.uint32, (4,)).tolist()) == summary, what
            for t in (d_col, d_keys, d_hit, d_lev, d_out, d_fb, d_terms, d_sum):
                assert bool((t[-GUARD_BYTES:] == 0x5A).all()), what
            # the inputs are unchanged (the colours: unless they are the output)
            assert np.array_equal(_payload(d_keys, np.uint32, (Hf, Wf)), case["keys"]), what
            assert np.array_equal(_payload(d_hit, np.int64, (Hf, Wf)), case["hit"]), what
            assert np.array_equal(_payload(d_lev, np.uint8, case["box"][1][::-1]), case["levels"].transpose(2, 1, 0)), what
            if mode == "alias":
                assert bool((d_out[:-GUARD_BYTES] == 0x7B).all()), what
            else:
                assert np.array_equal(R.bits(_payload(d_col, F32, (Hf, Wf, 3))), R.bits(case["color"])), what
    finally:
        ctx.close()


def test_a_frame_on_which_the_counting_launch_walks_several_tiles_per_wave(eng, vxo):
    """with a summary the launch is at most two workgroups of 16 waves per compute unit: 1990 x 262 is 2112 tiles of 64 x 4,
    more than the 2048 groups of four waves a device of 256 compute units gets, and neither side is a multiple of the tile; the
    same frame without a summary (one tile per workgroup) gives the same bits.  Through the Python mirror."""
    vx, torch = eng
    Wf, Hf = 1990, 262
    case = LC.random_case(Wf, Hf, False)
    color, terms, summary = LC.run_case(case)[:3]
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(case["world"], 8))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        args = (dev(case["color"]), dev(case["keys"].view(np.int32)), dev(case["hit"]), case["cam"])
        kw = dict(field=dev(case["levels"].transpose(2, 1, 0)), box=case["box"], **case["params"])
        counted = ctx.light_frame(*args, terms=True, **kw)
        plain = ctx.light_frame(*args, summary=False, **kw)
        torch.cuda.synchronize()
        assert tuple(counted.summary) == summary and min(summary) > 1000 and plain.summary is None and plain.terms is None
        for got in (counted, plain):
            assert np.array_equal(R.bits(got.color.cpu().numpy()), R.bits(color))
        assert np.array_equal(R.bits(counted.terms.cpu().numpy()), R.bits(terms))
    finally:
        ctx.close()


# ---- the whole path on rendered frames ---------------------------------------------------------------------------------
def _centre_voxel(vxo, dense, dims, factor, cam):
    """the voxel that the hit pixel nearest to the centroid of the frame's hit pixels shows (the oracle's hit AOV, unshaded)"""
    X, Y, Z = dims
    w = vxo.World.from_dense(dense, X, Y, Z, factor)
    hit = w.render(vxo.make_params(W, H, *cam, frame_number=3), fb=np.zeros((H, W, 4), np.uint8), want_hit=True, nthreads=16)["hit"]
    ys, xs = np.nonzero(hit >= 0)
    assert len(ys) > W * H // 5
    at = np.argmin((ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2)
    h = int(hit[ys[at], xs[at]])
    return h % X, h // X % Y, h // (X * Y)


def _scene(vxo, factor):
    """terrain with a roof plate six voxels above the surface point the frame's centre shows, the light box around it
    (smaller than the view), two emitters under the roof, and the edit that opens the roof"""
    X, Y, Z = dims = WORLDS[factor]
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    cam = helpers.camera("A", dims, vxo)
    cx, cy, cz = _centre_voxel(vxo, dense, dims, factor, cam)
    roof = [(helpers.BOX, 1, (cx - 12, cy + 6, cz - 12), (cx + 12, cy + 6, cz + 12))]
    hole = [(helpers.BOX, 0, (cx - 3, cy + 6, cz - 3), (cx + 3, cy + 6, cz + 3))]
    box = ((cx - 16, cy - 10, cz - 16), (32, 24, 32))
    emitters = [(cx, cy + 3, cz, 15), (cx + 5, cy + 4, cz - 4, 10)]
    return dict(dims=dims, dense=dense, cam=cam, roof=roof, hole=hole, box=box, emitters=emitters)


def _reference(vxo, scene, factor, ops):
    X, Y, Z = scene["dims"]
    dense = vxo_edit.apply_edits(scene["dense"], X, Y, Z, ops)
    vox = vxo_edit.voxels_from_dense(dense, X, Y, Z)
    w = vxo.World.from_dense(dense, X, Y, Z, factor)
    ref = w.render(vxo.make_params(W, H, *scene["cam"], frame_number=3, **SHADED), fb=np.zeros((H, W, 4), np.uint8), want_color=True,
                   want_hit=True, nthreads=16)
    field = ref_light.light_field(vox, *scene["box"], scene["emitters"])
    color, terms, summary, info = LF.light_frame(ref["color"], ref["hit"], scene["cam"], vox, field["levels"], scene["box"], LC.PARAMS)
    return dict(color=color, terms=terms, summary=summary, field=field, info=info)


def _device(vx, torch, ctx, scene, stream=None):
    pos, f, u, r = scene["cam"]
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.full((H, W), -7, dtype=torch.int64, device="cuda")
    opts = vx.RenderOptions(shadow=True, bounce_samples=1, bounce_all_hits=True, frame_number=3)
    ctx.RenderScreen(W, H, fb, pos, f, u, r, opts, color_aov=col, hit_aov=hit, stream=stream)
    keys = ctx.frame_guides(W, H, *scene["cam"], hit, stream=stream)
    field = ctx.light_field(*scene["box"], scene["emitters"], stream=stream)
    lit = ctx.light_frame(col, keys, hit, scene["cam"], field, fb=fb, terms=True, stream=stream, **LC.PARAMS)
    return lit, fb, field, (col, keys, hit)


def _assert_frame(got, want, what):
    lit, fb, field, _ = got
    assert np.array_equal(field.grid(), want["field"]["levels"]), what
    assert np.array_equal(R.bits(lit.color.cpu().numpy()), R.bits(want["color"])), what
    assert np.array_equal(R.bits(lit.terms.cpu().numpy()), R.bits(want["terms"])), what
    assert np.array_equal(fb.cpu().numpy(), R.bgra8(want["color"])), what
    assert tuple(lit.summary) == want["summary"], what


@pytest.fixture(scope="module")
def scenes(eng, vxo):
    """per brick edge: the scene, a context that holds its world with the roof, and the references before and after the hole"""
    vx, _ = eng
    out = {}
    for factor in sorted(WORLDS):
        scene = _scene(vxo, factor)
        ctx = new_ctx(vx)
        X, Y, Z = scene["dims"]
        upload(ctx, vxo.World.from_dense(scene["dense"], X, Y, Z, factor))
        ctx.edit_voxels(scene["roof"])
        out[factor] = (ctx, scene, _reference(vxo, scene, factor, scene["roof"]))
    yield out
    for ctx, _, _ in out.values():
        ctx.close()


@pytest.mark.parametrize("factor", sorted(WORLDS))
def test_render_guides_field_light_equals_the_restatement_on_the_oracle_frame(eng, vxo, scenes, factor):
    """and again after an edit that opens the roof and a relight: more sky reaches the ground under it"""
    vx, torch = eng
    ctx, scene, closed = scenes[factor]
    got = _device(vx, torch, ctx, scene)
    torch.cuda.synchronize()
    _assert_frame(got, closed, (factor, "roof"))
    hitn, in_box, occluded, dark = closed["summary"]
    print("light frame pipeline", factor, "hit, in_box, occluded, dark", closed["summary"])
    assert 0 < in_box < hitn and occluded > 0 and closed["terms"][..., 1].max() > 0  # the box is smaller than the view; an emitter shows
    try:
        ctx.edit_voxels(scene["hole"])
        opened = _reference(vxo, scene, factor, scene["roof"] + scene["hole"])
        got = _device(vx, torch, ctx, scene)
        torch.cuda.synchronize()
        _assert_frame(got, opened, (factor, "hole"))
        assert opened["field"]["summary"][4] > closed["field"]["summary"][4]  # sum_sky
        assert not np.array_equal(opened["color"], closed["color"])
    finally:
        ctx.edit_voxels(scene["roof"])  # the roof closed again for the tests that share the scene


def test_the_same_on_a_side_stream(eng, vxo, scenes):
    vx, torch = eng
    ctx, scene, closed = scenes[16]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = _device(vx, torch, ctx, scene, stream=side.cuda_stream)
    side.synchronize()
    _assert_frame(got, closed, "side stream")


def test_capture_and_replay_equals_the_eager_call(eng, vxo, scenes):
    """vxrt_light_frame captured in global mode on a side stream and replayed twice"""
    vx, torch = eng
    ctx, scene, closed = scenes[32]
    lit, fb, field, (col, keys, hit) = _device(vx, torch, ctx, scene)
    torch.cuda.synchronize()
    _assert_frame((lit, fb, field, None), closed, "eager")
    side = torch.cuda.Stream()
    out = torch.zeros_like(col)
    fb2 = torch.zeros_like(fb)
    terms = torch.zeros_like(col)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        res = ctx.light_frame(col, keys, hit, scene["cam"], field, out=out, fb=fb2, terms=terms, **LC.PARAMS)
    assert not out.any() and not fb2.any()  # capturing ran nothing
    for _ in range(2):
        out.zero_()
        fb2.zero_()
        terms.zero_()
        res._summary.fill_(77)
        with torch.cuda.stream(side):
            g.replay()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), lit.color.view(torch.int32)) and torch.equal(fb2, fb)
        assert torch.equal(terms.view(torch.int32), lit.terms.view(torch.int32))
        assert tuple(int(v) for v in res._summary.cpu()) == tuple(lit.summary)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order_with_nothing_written(eng, vxo, tmp_path):
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    n = 16 * 8
    col = torch.full((8, 16, 3), 0.5, dtype=torch.float32, device="cuda")
    keys = torch.full((n,), 0x1234, dtype=torch.int32, device="cuda")
    hit = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    levels = torch.full((64,), 0x33, dtype=torch.uint8, device="cuda")
    out = torch.full((8, 16, 3), 9.0, dtype=torch.float32, device="cuda")
    fb = torch.full((n,), 0x1234, dtype=torch.int32, device="cuda")
    terms = torch.full((8, 16, 3), 9.0, dtype=torch.float32, device="cuda")
    summary = torch.full((4,), 0x1234, dtype=torch.int32, device="cuda")
    nan, inf = float("nan"), float("inf")
    empty, streamed, world = vx.Context(0), vx.Context(0), new_ctx(vx)

    def err():
        return L.vxrt_last_error().decode()

    def call(h=empty._h, Wf=16, Hf=8, size=C.sizeof(N.LightFrameParams), params=True, flags=3, outside=0xF0, reserved=0, sky_floor=0.5,
             block=(1.0, 1.0, 1.0), curve=(0.4, 0.6, 0.8, 1.0), bad=None, dims=(4, 4, 4), origin=(0, 0, 0), cp=col.data_ptr(),
             kp=keys.data_ptr(), hp=hit.data_ptr(), op=out.data_ptr()):
        p = N.LightFrameParams(struct_size=size, ortho=0, flags=flags, outside_level=outside, sky_floor=sky_floor, reserved_=reserved)
        p.block_color, p.ao_curve = (C.c_float * 3)(*block), (C.c_float * 4)(*curve)
        p.cam.origin, p.cam.fwd, p.cam.up, p.cam.right = ((C.c_float * 3)(*v) for v in ((1, 2, 3), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
        if bad:
            field, k, v = bad
            getattr(p.cam, field)[k] = v
        p.box_origin, p.box_dims = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims)
        return L.vxrt_light_frame(h, Wf, Hf, cp, kp, hp, levels.data_ptr(), C.byref(p) if params else None, op, fb.data_ptr(),
                                  terms.data_ptr(), summary.data_ptr(), None)

    try:
        # each call has the earlier faults mended and all the later ones still in it; the context holds no world
        later = dict(size=8, flags=4, sky_floor=nan, curve=(0.4, 0.6, 0.8, -1.0), bad=("fwd", 1, nan), dims=(0, 4, 4), cp=None)
        assert call(h=None, Wf=0, **later) == -1 and "ctx" in err()
        for Wf, Hf in ((0, 8), (16, 0), (65536, 1), (1, 65536), (8193, 8192)):
            assert call(Wf=Wf, Hf=Hf, **later) == -1 and "W, H" in err()
        assert call(**later) == -1 and "size" in err()
        later.pop("size")
        assert call(params=False, cp=None) == -1 and "size" in err()
        for flags in (4, 7, 1 << 31):
            assert call(**dict(later, flags=flags)) == -1 and "flags" in err()
        later.pop("flags")
        assert call(outside=0x100, **later) == -1 and "flags" in err()
        assert call(reserved=1, **later) == -1 and "flags" in err()
        for s in (nan, -0.5, 1.5, inf):
            assert call(**dict(later, sky_floor=s)) == -1 and "sky_floor" in err()
        later.pop("sky_floor")
        for kw in (dict(curve=(0.4, 0.6, 0.8, -1.0)), dict(curve=(nan, 0.6, 0.8, 1.0)), dict(curve=(0.4, inf, 0.8, 1.0)), dict(block=(1.0, -1.0, 1.0)),
                   dict(block=(1.0, 1.0, nan)), dict(block=(inf, 1.0, 1.0))):
            assert call(**dict(later, **kw)) == -1 and "block_color or ao_curve" in err()
        later.pop("curve")
        for field in ("origin", "fwd", "up", "right"):
            for k, v in ((0, nan), (2, inf), (1, -inf)):
                assert call(**dict(later, bad=(field, k, v))) == -1 and "non-finite" in err()
        later.pop("bad")
        for kw in (dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(1 << 10, 1 << 10, (1 << 8) + 1)),
                   dict(dims=(4, 4, 4), origin=(0, 2 ** 31 - 4, 0))):
            assert call(**dict(later, **kw)) == -1 and "box" in err()
        later.pop("dims")
        for kw in (dict(cp=None), dict(kp=None), dict(hp=None), dict(op=None)):
            assert call(**kw) == -1 and "NULL" in err()
        assert call() == -3 and "no world" in err()  # VXRT_ERR_NO_WORLD
        # a streamed world is a cache: it is not lit.  (The last refusal, a world axis longer than 2^24 voxels, has no case: the
        # tables hold at most 65535 cells of 32 voxels per axis, so no such world can be made resident.)
        w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16)
        upload(world, w)
        path = str(tmp_path / "w.vxb")
        world.save_world(path)
        streamed.stream_open(path, 1000)
        assert call(h=streamed._h) == -1 and "streamed" in err()
        torch.cuda.synchronize()
        assert bool((out == 9.0).all()) and bool((terms == 9.0).all()) and bool((fb == 0x1234).all()) and bool((summary == 0x1234).all())
        assert bool((col == 0.5).all()) and bool((keys == 0x1234).all()) and bool((hit == 5).all()) and bool((levels == 0x33).all())
        # and the same arguments on a resident world are accepted (the keys are no guide keys of this camera: only that the
        # call runs, counts every pixel as a hit and writes every output)
        assert call(h=world._h) == 0
        torch.cuda.synchronize()
        assert summary.tolist()[0] == n and not bool((out == 9.0).any()) and not bool((terms == 9.0).any()) and not bool((fb == 0x1234).any())
    finally:
        for c in (empty, streamed, world):
            c.close()


def test_strided_tensors_are_refused_and_left_unchanged(eng, vxo):
    vx, torch = eng
    Wf, Hf = 16, 8
    n = Wf * Hf
    cam = ((1.0, 2.0, 3.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    col = torch.full((Hf, Wf, 3), 0.5, dtype=torch.float32, device="cuda")
    keys = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    hit = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    out = torch.full((Hf, Wf, 6), 9.0, dtype=torch.float32, device="cuda")
    fb = torch.full((2 * n,), 0x1234, dtype=torch.int32, device="cuda")
    levels = torch.zeros(128, dtype=torch.uint8, device="cuda")
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(LC.plate_world(), 8))
        for kw in (dict(out=out[:, :, ::2]), dict(fb=fb[::2]), dict(terms=out[:, :, ::2]), dict(field=levels[::2], box=((0, 0, 0), (4, 4, 4))),
                   dict(field=levels, box=((0, 0, 0), (4, 4, 9)))):
            with pytest.raises(ValueError):
                ctx.light_frame(col, keys[:n], hit[:n], cam, **kw)
        for k, h in ((keys[::2], hit[:n]), (keys[:n], hit[::2])):
            with pytest.raises(ValueError):
                ctx.light_frame(col, k, h, cam)
        torch.cuda.synchronize()
        assert bool((out == 9.0).all()) and bool((fb == 0x1234).all())
        got = ctx.light_frame(col, keys[:n], hit[:n], cam, terms=True)  # every pixel a miss: copied
        assert tuple(got.summary) == (0, 0, 0, 0) and bool((got.color == 0.5).all()) and not bool(got.terms.any())
    finally:
        ctx.close()


# ---- the example ---------------------------------------------------------------------------------------------------------
def test_headless_example_lit_line(eng, vxo, tmp_path):
    """examples/voxelapp_headless on a path of three poses with "0 lit <box> 0.25 <two emitters>" and "2 lit off": the summary
    lines of frames 0 and 1 are those of the Python path on the same world, the dumped PPMs the lit frames, and frame 2 is
    the plain frame"""
    vx, torch = eng
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge, Wf, Hf = 256, 64, 48
    f32 = lambda v: tuple(float(F32(x)) for x in v)  # binary32 values: their repr reads back as the same binary32
    eulers = [f32((-0.45 + 0.005 * j, 0.7 + 0.01 * j, 0.0)) for j in range(3)]
    positions = [f32((edge * 0.25 + 0.5 * j, edge * 0.9 - 0.25 * j, edge * 0.25 + 0.25 * j)) for j in range(3)]
    (tmp_path / "path.txt").write_text("".join("%r %r %r %r %r %r\n" % (*p, *e) for p, e in zip(positions, eulers)))
    box = ((60, 150, 60), (96, 90, 96))
    emitters = [(80, 216, 80, 15), (100, 200, 110, 12)]
    (tmp_path / "script.txt").write_text("0 lit %d %d %d %d %d %d 0.25 %s\n2 lit off\n" % (*box[0], *box[1], " ".join("%d %d %d %d" % e for e in emitters)))
    out = subprocess.run([exe, str(edge), "3", str(tmp_path / "lf"), str(Wf), str(Hf), "2", str(tmp_path / "path.txt"), "1", "1", "1",
                          "0x0x0", str(tmp_path / "script.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [x for x in out.stdout.splitlines() if x.startswith("lit ")]
    assert len(lines) == 2, out.stdout

    dense = gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(dense, edge, edge, edge, 32))
        field = ctx.light_field(*box, emitters)
        for j in range(3):
            f, u, r = vxo.get_directions(eulers[j])
            cam = (positions[j], f, u, r)
            fb = torch.zeros((Hf, Wf, 4), dtype=torch.uint8, device="cuda")
            col = torch.zeros((Hf, Wf, 3), dtype=torch.float32, device="cuda")
            hit = torch.zeros((Hf, Wf), dtype=torch.int64, device="cuda")
            ctx.RenderScreen(Wf, Hf, fb, *cam, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=j), color_aov=col, hit_aov=hit)
            if j < 2:
                keys = ctx.frame_guides(Wf, Hf, *cam, hit)
                got = ctx.light_frame(col, keys, hit, cam, field, sky_floor=0.25, fb=fb)
                s = got.summary
                assert lines[j] == "lit frame %d hit %d in_box %d occluded %d dark %d" % (j, *s), (j, lines)
                assert s.hit > 100
            torch.cuda.synchronize()
            ppm = open(tmp_path / ("lf_%04d.ppm" % j), "rb").read()
            rgb = np.frombuffer(ppm[-Wf * Hf * 3:], np.uint8).reshape(Hf, Wf, 3)
            assert np.array_equal(rgb, fb.cpu().numpy()[..., 2::-1]), j
    finally:
        ctx.close()
