"""The frame denoiser on the device (include/vxrt.h, vxrt_frame_guides / vxrt_denoise_frame): the filtered colours and the
BGRA8 frame bit-equal to tests/ref_denoise.py on the random frames of the host tests, for every iteration count and with and
without the colour stop, the output aliasing the input, guard words behind the outputs, the keys and the workspace; the guide
keys bit-equal on renders of small procedural worlds, perspective and ortho, at every brick edge; the whole path -- render
with both AOVs, guides, filter -- bit-equal to the restatement applied to the oracle's frame, on a side stream, after an edit
and from a captured graph; every refusal in the documented order with nothing written; and the headless example's denoise
line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import vxo_edit
from tests import helpers
from tests import ref_denoise as R
from tests.helpers import eng, gen_dense, new_ctx, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A
F32 = np.float32
W, H = 160, 96
SHADED = dict(shadow=1, bounce_samples=1, bounce_all_hits=1)
_CACHE = {}


def _want(Wf, Hf, n, k):
    key = (Wf, Hf, n, k)
    if key not in _CACHE:
        c, keys = R.random_frame(Wf, Hf)
        _CACHE[key] = R.denoise_np(c, keys, n, k)
    return _CACHE[key]


def _guarded(torch, n, dtype, fill=0):
    """a tensor of n elements with 64 guard words behind it: (the n elements, the whole tensor)"""
    per = 4 // torch.empty(0, dtype=dtype).element_size()
    t = torch.full((n + 64 * per,), fill, dtype=dtype, device="cuda")
    t.view(torch.int32)[-64:] = GUARD
    return t[:n], t


def _guards_ok(torch, whole):
    return bool((whole.view(torch.int32)[-64:] == GUARD).all())


@pytest.fixture(scope="module")
def ctx(eng):
    vx, _ = eng
    c = new_ctx(vx)
    yield c
    c.close()


@pytest.mark.parametrize("Wf,Hf", R.FRAMES)
def test_filter_equals_the_restatement(eng, ctx, Wf, Hf):
    """float and BGRA8 outputs for iterations 1 .. 6 with and without the colour stop; the output aliasing the input on every
    other case; guards behind the outputs, the keys and the workspace; the input and the keys unchanged"""
    vx, torch = eng
    c, keys = R.random_frame(Wf, Hf)
    n = Wf * Hf
    assert ctx.denoise_workspace_bytes(Wf, Hf) == R.workspace_bytes(Wf, Hf) == 32 * n
    for it in R.ITERATIONS:
        for k in R.SCALES:
            alias = (it + (k > 0)) % 2 == 1
            cin, cin_all = _guarded(torch, 3 * n, torch.float32)
            kk, kk_all = _guarded(torch, n, torch.int32)
            out, out_all = _guarded(torch, 3 * n, torch.float32, float("nan"))
            fb, fb_all = _guarded(torch, 4 * n, torch.uint8, 7)
            work, work_all = _guarded(torch, 32 * n, torch.uint8, 0xA5)
            cin.copy_(torch.from_numpy(c.reshape(-1)))
            kk.copy_(torch.from_numpy(keys.view(np.int32).reshape(-1)))
            src = cin.view(Hf, Wf, 3)
            got = ctx.denoise_frame(src, kk, it, k, out=src if alias else out.view(Hf, Wf, 3), fb=fb, work=work)
            torch.cuda.synchronize()
            want = _want(Wf, Hf, it, k)
            what = (Wf, Hf, it, k, alias)
            assert np.array_equal(R.bits(got.cpu().numpy()), R.bits(want)), what
            assert np.array_equal(fb.cpu().numpy().reshape(Hf, Wf, 4), R.bgra8(want)), what
            for whole in (cin_all, kk_all, out_all, fb_all, work_all):
                assert _guards_ok(torch, whole), what
            assert np.array_equal(kk.cpu().numpy().view(np.uint32).reshape(Hf, Wf), keys), what
            if alias:
                assert bool(torch.isnan(out).all()), what
            else:
                assert np.array_equal(R.bits(cin.cpu().numpy().reshape(Hf, Wf, 3)), R.bits(c)), what
            if it == 1 and not alias:  # one fused launch touches no workspace
                assert bool((work == 0xA5).all()), what


# ---- guide keys and the whole path on rendered frames ------------------------------------------------------------------
WORLDS = {8: (128, 128, 128), 16: (128, 128, 128), 32: (256, 256, 256)}
ORTHO_SIZE = (40.0, 30.0)


@pytest.fixture(scope="module")
def scenes(eng, vxo):
    vx, _ = eng
    out = {}
    for f, dims in WORLDS.items():
        w = vxo.World.generate(vxo.GEN_INT_TERRAIN, *dims, f)
        c = new_ctx(vx)
        c.SetOrthoWindowSize(*ORTHO_SIZE)
        upload(c, w)
        out[f] = (c, w)
    yield out
    for c, _ in out.values():
        c.close()


def _render(vx, torch, ctx, cam, ortho, frame_number=3, stream=None):
    pos, f, u, r = cam
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.full((H, W), -7, dtype=torch.int64, device="cuda")
    opts = vx.RenderOptions(shadow=True, bounce_samples=1, bounce_all_hits=True, ortho=ortho, frame_number=frame_number)
    ctx.RenderScreen(W, H, fb, pos, f, u, r, opts, color_aov=col, hit_aov=hit, stream=stream)
    return fb, col, hit


def _oracle(vxo, w, cam, ortho, frame_number=3):
    pos, f, u, r = cam
    p = vxo.make_params(W, H, pos, f, u, r, frame_number=frame_number, ortho=int(ortho), ortho_size=ORTHO_SIZE, **SHADED)
    return w.render(p, fb=np.zeros((H, W, 4), np.uint8), want_color=True, want_hit=True, nthreads=16)


def _ref_keys(w, cam, ortho, hit):
    pos, f, u, r = cam
    o, d = R.primary_rays(W, H, pos, f, u, r, ortho=ortho, ortho_size=ORTHO_SIZE)
    return R.keys_np(hit, w.dims, o, d)


@pytest.mark.parametrize("factor", sorted(WORLDS))
@pytest.mark.parametrize("ortho", (False, True))
def test_keys_equal_the_restatement_on_rendered_frames(eng, vxo, scenes, factor, ortho):
    vx, torch = eng
    ctx, w = scenes[factor]
    for name in "AD":
        cam = helpers.camera(name, w.dims, vxo)
        _, _, hit = _render(vx, torch, ctx, cam, ortho)
        keys_all = torch.full((H * W + 64,), GUARD, dtype=torch.int32, device="cuda")
        keys = ctx.frame_guides(W, H, *cam, hit, ortho=ortho, out=keys_all)
        torch.cuda.synchronize()
        h = hit.cpu().numpy()
        want = _ref_keys(w, cam, ortho, h)
        got = keys.cpu().numpy().view(np.uint32)
        print("keys", factor, ortho, name, "hit pixels", int((h >= 0).sum()), "faces", len(np.unique(want)))
        assert np.array_equal(got, want), (factor, ortho, name)
        assert _guards_ok(torch, keys_all) and np.array_equal(got != 0, h >= 0)
        assert ortho or name == "D" or len(np.unique(want)) > 20


def _pipeline(vx, torch, ctx, cam, ortho, n, k, stream=None, frame_number=3):
    fb, col, hit = _render(vx, torch, ctx, cam, ortho, frame_number, stream)
    keys = ctx.frame_guides(W, H, *cam, hit, ortho=ortho, stream=stream)
    out = ctx.denoise_frame(col, keys, n, k, fb=fb, stream=stream)
    return fb, col, hit, keys, out


def _assert_pipeline(vxo, w, cam, ortho, n, k, got, what, frame_number=3):
    """the restatement applied to the oracle's frame"""
    fb, col, hit, keys, out = (t.cpu().numpy() for t in got)
    ref = _oracle(vxo, w, cam, ortho, frame_number)
    assert np.array_equal(hit, ref["hit"]), what
    diff = np.abs(col.astype(np.float64) - ref["color"])
    print("pipeline", what, "colour AOV against the oracle: max abs diff", float(np.nanmax(diff)), "unequal bits",
          int((R.bits(col) != R.bits(ref["color"])).sum()))
    want_keys = _ref_keys(w, cam, ortho, ref["hit"])
    assert np.array_equal(keys.view(np.uint32), want_keys), what
    want = R.denoise_np(ref["color"], want_keys, n, k)
    assert np.array_equal(R.bits(out), R.bits(want)), what
    assert np.array_equal(fb, R.bgra8(want)), what
    assert not np.array_equal(R.bits(want), R.bits(ref["color"])), what  # the filter did something


def test_render_guides_denoise_equals_the_restatement_on_the_oracle_frame(eng, vxo, scenes):
    vx, torch = eng
    for factor, name, ortho, n, k in ((32, "A", False, 4, 0.0), (16, "A", False, 5, 0.75), (8, "A", True, 2, 0.0)):
        ctx, w = scenes[factor]
        cam = helpers.camera(name, w.dims, vxo)
        got = _pipeline(vx, torch, ctx, cam, ortho, n, k)
        torch.cuda.synchronize()
        _assert_pipeline(vxo, w, cam, ortho, n, k, got, (factor, name, ortho, n, k))


def test_the_same_on_a_side_stream(eng, vxo, scenes):
    vx, torch = eng
    ctx, w = scenes[16]
    cam = helpers.camera("A", w.dims, vxo)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = _pipeline(vx, torch, ctx, cam, False, 3, 0.75, stream=side.cuda_stream)
    side.synchronize()
    _assert_pipeline(vxo, w, cam, False, 3, 0.75, got, "side stream")


def test_the_same_after_an_edit_that_changes_the_hit_aov(eng, vxo):
    vx, torch = eng
    X = Y = Z = 128
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx = new_ctx(vx)
    try:
        before = vxo.World.from_dense(dense, X, Y, Z, 16)
        upload(ctx, before)
        cam = helpers.camera("A", before.dims, vxo)
        first = _pipeline(vx, torch, ctx, cam, False, 3, 0.0)
        torch.cuda.synchronize()
        _assert_pipeline(vxo, before, cam, False, 3, 0.0, first, "before the edit")
        ops = [(helpers.SPHERE, 0, (64, 60, 64), (20, 0, 0)), (helpers.BOX, 1, (40, 70, 40), (60, 90, 50))]
        ctx.edit_voxels(ops)
        after = vxo.World.from_dense(vxo_edit.apply_edits(dense, X, Y, Z, ops), X, Y, Z, 16)
        second = _pipeline(vx, torch, ctx, cam, False, 3, 0.0)
        torch.cuda.synchronize()
        assert not torch.equal(first[2], second[2]) and not torch.equal(first[3], second[3])
        _assert_pipeline(vxo, after, cam, False, 3, 0.0, second, "after the edit")
    finally:
        ctx.close()


def test_capture_and_replay_of_guides_and_denoise_equals_the_eager_result(eng, vxo, scenes):
    vx, torch = eng
    ctx, w = scenes[32]
    cam = helpers.camera("A", w.dims, vxo)
    fb, col, hit = _render(vx, torch, ctx, cam, False)
    keys_e = ctx.frame_guides(W, H, *cam, hit)
    out_e = ctx.denoise_frame(col, keys_e, 4, 0.75)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    keys = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(col)
    fb2 = torch.zeros_like(fb)
    work = torch.zeros(ctx.denoise_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.frame_guides(W, H, *cam, hit, out=keys)
        ctx.denoise_frame(col, keys, 4, 0.75, out=out, fb=fb2, work=work)
    assert not keys.any() and not out.any()  # capturing ran nothing
    for _ in range(2):
        keys.zero_()
        out.zero_()
        with torch.cuda.stream(side):
            g.replay()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(keys.view(H, W), keys_e) and torch.equal(out.view(torch.int32), out_e.view(torch.int32))
        assert np.array_equal(fb2.cpu().numpy(), R.bgra8(out_e.cpu().numpy()))


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order_with_nothing_written(eng, vxo, scenes):
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    ctx, w = scenes[16]
    empty = new_ctx(vx)  # no world resident
    try:
        n = 16 * 8
        col = torch.full((8, 16, 3), 0.5, dtype=torch.float32, device="cuda")
        keys = torch.full((n,), 0x1234, dtype=torch.int32, device="cuda")
        hit = torch.zeros(n, dtype=torch.int64, device="cuda")
        out = torch.full((8, 16, 3), 9.0, dtype=torch.float32, device="cuda")
        fb = torch.full((n,), 0x1234, dtype=torch.int32, device="cuda")
        work = torch.full((32 * n,), 0xA5, dtype=torch.uint8, device="cuda")
        v = (C.c_float * 3)(1.0, 0.0, 0.0)
        nan = float("nan")

        def err():
            return L.vxrt_last_error().decode()

        def guides(h=ctx._h, Wf=16, Hf=8, o=v, f=v, u=v, r=v, hp=hit.data_ptr(), kp=keys.data_ptr()):
            return L.vxrt_frame_guides(h, Wf, Hf, o, f, u, r, 0, hp, kp, None)

        def denoise(h=ctx._h, Wf=16, Hf=8, cp=col.data_ptr(), kp=keys.data_ptr(), size=16, it=2, k=0.0, params=True, wp=work.data_ptr(),
                    op=out.data_ptr()):
            p = N.DenoiseParams(struct_size=size, iterations=it, color_scale=k)
            return L.vxrt_denoise_frame(h, Wf, Hf, cp, kp, C.byref(p) if params else None, wp, op, fb.data_ptr(), None)

        # guides: each call has the earlier faults mended and all the later ones still in it
        assert guides(h=None, Wf=0, o=None, kp=None) == -1 and "ctx" in err()
        assert guides(h=empty._h, Wf=0, o=None, kp=None) == -1 and "no world" in err()
        for Wf, Hf in ((0, 8), (16, 0), (65536, 1), (1, 65536), (8193, 8192)):
            assert guides(Wf=Wf, Hf=Hf, o=None, kp=None) == -1 and "W, H" in err()
        for kw in (dict(o=None), dict(f=None), dict(u=None), dict(r=None), dict(hp=None), dict(kp=None)):
            assert guides(**kw) == -1 and "NULL" in err()
        assert guides() == 0
        # the filter
        assert denoise(h=None, Wf=0, size=8, it=0, k=nan, cp=None) == -1 and "ctx" in err()
        for Wf, Hf in ((0, 8), (16, 0), (65536, 1), (1, 65536), (8193, 8192)):
            assert denoise(Wf=Wf, Hf=Hf, size=8, it=0, k=nan, cp=None) == -1 and "W, H" in err()
        assert denoise(size=8, it=0, k=nan, cp=None) == -1 and "size" in err()
        assert denoise(params=False, cp=None) == -1 and "size" in err()
        for it in (0, 7, -1):
            assert denoise(it=it, k=nan, cp=None) == -1 and "iterations" in err()
        for k in (nan, -1.0, -0.5):
            assert denoise(k=k, cp=None) == -1 and "color_scale" in err()
        for kw in (dict(cp=None), dict(kp=None), dict(wp=None), dict(op=None)):
            assert denoise(**kw) == -1 and "NULL" in err()
        torch.cuda.synchronize()
        # nothing was written by any refused call (the one accepted guides call wrote the keys)
        assert bool((out == 9.0).all()) and bool((fb == 0x1234).all()) and bool((work == 0xA5).all()) and bool((col == 0.5).all())
        assert not bool((keys == 0x1234).any())
        assert denoise(k=0.0) == 0 and denoise(k=float("inf")) == 0  # a context without a world filters too (below)
        assert L.vxrt_denoise_frame(empty._h, 16, 8, col.data_ptr(), keys.data_ptr(),
                                    C.byref(N.DenoiseParams(struct_size=16, iterations=1, color_scale=0.0)), work.data_ptr(),
                                    out.data_ptr(), None, None) == 0
        torch.cuda.synchronize()
        assert ctx.denoise_workspace_bytes(0, 8) == 0 and ctx.denoise_workspace_bytes(8193, 8192) == 0
        assert ctx.denoise_workspace_bytes(8192, 8192) == 1 << 31
    finally:
        empty.close()


def test_strided_tensors_are_refused_and_left_unchanged(eng, scenes):
    """frame_guides and denoise_frame hand the library the tensors' addresses as dense buffers: a tensor with a stride is
    refused before the library is called, and the dense part of the same memory is accepted"""
    vx, torch = eng
    ctx, _ = scenes[min(WORLDS)]
    Wf, Hf = 16, 8
    n = Wf * Hf
    cam = ((1.0, 2.0, 3.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    hit = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")  # every pixel a miss
    keys = torch.full((2 * n,), 0x1234, dtype=torch.int32, device="cuda")
    col = torch.full((Hf, Wf, 3), 0.5, dtype=torch.float32, device="cuda")
    out = torch.full((Hf, Wf, 6), 9.0, dtype=torch.float32, device="cuda")
    fb = torch.full((2 * n,), 0x1234, dtype=torch.int32, device="cuda")
    work = torch.full((2 * ctx.denoise_workspace_bytes(Wf, Hf),), 0xA5, dtype=torch.uint8, device="cuda")
    for h, k in ((hit[:n], keys[::2]), (hit[::2], keys[:n])):
        with pytest.raises(ValueError):
            ctx.frame_guides(Wf, Hf, *cam, h, out=k)
    for kw in (dict(out=out[:, :, ::2]), dict(fb=fb[::2]), dict(work=work[::2])):
        with pytest.raises(ValueError):
            ctx.denoise_frame(col, keys[:n], 2, 0.0, **kw)
    with pytest.raises(ValueError):
        ctx.denoise_frame(col, keys[::2], 2, 0.0)
    torch.cuda.synchronize()
    assert bool((keys == 0x1234).all()) and bool((out == 9.0).all()) and bool((fb == 0x1234).all()) and bool((work == 0xA5).all())
    got = ctx.frame_guides(Wf, Hf, *cam, hit[:n], out=keys[:n])
    torch.cuda.synchronize()
    assert got.shape == (Hf, Wf) and not bool(got.any()) and bool((keys[n:] == 0x1234).all())


def test_no_world_reaches_the_refusal_of_an_axis_longer_than_2_24_voxels(eng):
    """the last refusal of vxrt_frame_guides guards the binary32 form of a face plane; the world paths admit at most 65535
    coarse cells of at most 32 voxels per axis (below 2^21), so no resident world can reach it: a longer world is refused
    where it would be made"""
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        with pytest.raises(vx.VxrtError, match="coarse dimensions"):
            ctx.build_world(2, (1 << 24) + 256, 256, 256, 32)
        with pytest.raises(vx.VxrtError, match="no world"):
            ctx.frame_guides(16, 8, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), torch.zeros(128, dtype=torch.int64, device="cuda"))
    finally:
        ctx.close()


# ---- the example ---------------------------------------------------------------------------------------------------------
def test_headless_example_denoise_line(vxo, tmp_path):
    """examples/voxelapp_headless with "0 denoise 3 0.5" then "2 denoise 0": frames 0 and 1 are denoised (summary lines,
    the dumped PPMs are the filtered frames: the restatement applied to the oracle's frame), frame 2 is the plain frame"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge, Wf, Hf = 256, 64, 48
    sf = tmp_path / "script.txt"
    sf.write_text("0 denoise 3 0.5\n2 denoise 0\n")
    out = subprocess.run([exe, str(edge), "3", str(tmp_path / "dn"), str(Wf), str(Hf), "2", "-", "1", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [x for x in out.stdout.splitlines() if x.startswith("denoise ")]
    assert len(lines) == 2 and lines[0].startswith("denoise frame 0 iterations 3 color_scale 0.5 hit ") and "frame 1" in lines[1]
    w = vxo.World.from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge, 32)
    pos = (edge * 0.25, edge * 0.9, edge * 0.25)
    f, u, r = vxo.get_directions((-0.45, 0.7, 0.0))
    for frame in range(3):
        p = vxo.make_params(Wf, Hf, pos, f, u, r, frame_number=frame, shadow=1, bounce_samples=1)
        ref = w.render(p, fb=np.zeros((Hf, Wf, 4), np.uint8), want_color=True, want_hit=True, nthreads=16)
        want = ref["fb"]
        if frame < 2:
            o, d = R.primary_rays(Wf, Hf, pos, f, u, r)
            keys = R.keys_np(ref["hit"], w.dims, o, d)
            want = R.bgra8(R.denoise_np(ref["color"], keys, 3, 0.5))
            fields = lines[frame].split()
            assert int(fields[fields.index("hit") + 1]) == int((keys != 0).sum()) > 100
            assert int(fields[fields.index("faces") + 1]) == len(np.unique(keys[keys != 0]))
        ppm = open(tmp_path / ("dn_%04d.ppm" % frame), "rb").read()
        rgb = np.frombuffer(ppm[-Wf * Hf * 3:], np.uint8).reshape(Hf, Wf, 3)
        assert np.array_equal(rgb, want[..., 2::-1]), frame
