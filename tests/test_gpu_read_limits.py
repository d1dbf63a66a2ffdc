"""Region reads, surface extraction and the frame denoiser on the device at the limits of their launches: the cases of
tests/read_limit_cases.py, each bit for bit against oracle/ref_region.py, tests/ref_surface.py or tests/ref_denoise.py, or
against an identity that tests/test_read_limits_host.py holds against them: reads of 2^21 workgroups on the second grid axis
(along z with surplus workgroups, and along rows of 2^26 words), every value of zsteps, every lane mapping of a row; the
surface scan with 72 groups a thread and the summary's counters at 6 * 2^27 quads; frames of 65535 pixels a side and of
nearly 2^26 pixels, NaN, infinite, negative-zero and denormal operands, guide keys of hit indices past 2^32 and an output
that overlaps the input in part.  The large results are compared on the device; every output has guard words behind it."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_region
from tests import read_limit_cases as F
from tests import ref_denoise as RD
from tests import ref_surface as RS
from tests import helpers
from tests.helpers import eng, new_ctx, upload
from tests.test_gpu_denoise import _guarded, _guards_ok
from tests.test_gpu_surface import _assert_equal, _summary, _u32

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
CANON = 0x7FC00000


def _ctx(vx, vxo, vox, factor):
    ctx = vx.Context(0)
    upload(ctx, vxo.World.from_voxels(np.asarray(vox), factor))
    return ctx


def _read(torch, ctx, o, d):
    """the words of a read into a buffer pre-filled with the guard word: (the words, the guard words behind them)"""
    n = F.region_words(d)
    buf = torch.full((n + 64,), GUARD, dtype=torch.int32, device="cuda")
    got = ctx.read_region(o, d, out=buf)
    torch.cuda.synchronize()
    assert got.numel() == n and got.data_ptr() == buf.data_ptr()
    return buf[:n], buf[n:]


# ---- region reads
def test_a_read_on_the_second_grid_axis_along_z(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    world, o, d = F.small_world(), F.ALONG_Z_ORIGIN, F.ALONG_Z_DIMS
    a = F.read_launch(d, caps)
    assert a.gy == 3 and a.surplus > 0  # reached: three grid rows, the last with workgroups past the box
    want = F.along_z_nonzero(world)
    ctx = _ctx(vx, vxo, world, 8)
    try:
        words, guard = _read(torch, ctx, o, d)
        nz = torch.nonzero(words).flatten()
        print("along z: nonzero words", int(nz.numel()), "of", words.numel())
        assert np.array_equal(nz.cpu().numpy(), want)
        assert bool((words[nz] == 1).all()) and bool((guard == GUARD).all())
    finally:
        ctx.close()


def test_a_read_on_the_second_grid_axis_along_rows(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    world, o, d = F.small_world(), F.ALONG_ROWS_ORIGIN, F.ALONG_ROWS_DIMS
    a = F.read_launch(d, caps)
    assert a.gy == 2 and a.nxc == caps["grid_2d_x"] and a.wpr == 1 << 26
    tail = F.along_rows_tail(world)
    ctx = _ctx(vx, vxo, world, 8)
    try:
        words, guard = _read(torch, ctx, o, d)
        rows = words.view(2, a.wpr)
        got = rows[:, -F.ALONG_ROWS_TAIL:].cpu().numpy().view(np.uint32)
        count = int(torch.count_nonzero(words))
        print("along rows: nonzero words", count, "tail", got.tolist())
        assert np.array_equal(got, tail) and count == np.count_nonzero(tail) > 3  # zeros, then the world's two rows
        assert bool((guard == GUARD).all())
        del words, rows
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def _assert_read(torch, ctx, world, o, d):
    want = ref_region.read_region(world, o, d)
    words, guard = _read(torch, ctx, o, d)
    got = words.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != F.pack_region(want))
    print("read", o, d, "set", int(want.sum()), "wrong words", len(bad), bad[:4].tolist())
    assert len(bad) == 0 and bool((guard == GUARD).all()), (o, d)
    return want


def test_every_zsteps_of_the_ladder(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    assert F.ladder_zsteps(caps) == [1, 2, 4, 8]  # reached: one box for each value
    world = F.small_world()
    ctx = _ctx(vx, vxo, world, 8)
    try:
        for o, d in F.LADDER_BOXES:
            assert d[2] % (4 * F.read_launch(d, caps).zsteps) != 0
            want = _assert_read(torch, ctx, world, o, d)
            assert want.any() and not want.all()
    finally:
        ctx.close()


def test_every_lane_mapping_of_a_row(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    m = [F.read_launch(d, caps) for _, d in F.MAPPING_BOXES]
    assert {x.L for x in m} == {8, 16, 32, 64} and {x.nxc for x in m} == {1, 2, 3}  # reached
    world = F.wide_world()
    ctx = _ctx(vx, vxo, world, F.WIDE_WORLD[3])
    try:
        for k, (o, d) in enumerate(F.MAPPING_BOXES):
            want = _assert_read(torch, ctx, world, o, d)
            assert want.any() and not want.all()
            if k in F.MAPPING_HOST:
                assert np.array_equal(ctx.read_region_host(o, d), want), (o, d)
    finally:
        ctx.close()


# ---- surfaces
def test_the_scan_with_72_groups_a_thread(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    assert F.surf_share(F.SHARE_DIMS, caps) == (18432, 72)
    own = F.share_reference()
    assert len(own.quads) > 100000
    ctx = _ctx(vx, vxo, F.share_world(), 8)
    try:
        for origin in F.SHARE_ORIGINS:
            want = F.translated(own, F.share_offset(origin))
            for mode in (RS.CAP, RS.OPEN):
                got = ctx.extract_surface(origin, F.SHARE_DIMS, mode, triangles=True)
                _assert_equal(got, want, (origin, mode))
                del got
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def test_the_counters_of_the_checkerboard(eng, vxo):
    vx, torch = eng
    dims = F.CHECKER_WORLD[:3]
    want = F.checker_summary(dims)
    assert want[2] == 6 << 27
    thin = RS.extract(F.checker(F.CHECKER_THIN), (0, 0, 0), F.CHECKER_THIN, RS.CAP)
    n0 = int(thin.summary[10])
    assert n0 == max(F.CHECKER_CAPACITIES)
    ctx = vx.Context(0)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, *F.CHECKER_WORLD)
        rows = torch.from_numpy(F.checker_stamp_rows(dims).view(np.int32).copy()).cuda()
        bits = rows.reshape(-1, 1).expand(-1, dims[0] // 32).contiguous().view(-1)
        st = ctx.edit_stamps([vx.Stamp((0, 0, 0), bits, 0, dims)])
        assert st.bricks_live == dims[0] * dims[1] * dims[2] // 32 ** 3
        del bits, rows
        L, h = ctx._L, ctx._h
        work = torch.zeros(ctx.surface_workspace_bytes(dims), dtype=torch.uint8, device="cuda")
        o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*dims)
        for mode in (RS.CAP, RS.OPEN):
            for cap in (0,) + F.CHECKER_CAPACITIES:
                q = torch.full((2 * cap + 8,), GUARD, dtype=torch.int32, device="cuda")
                summ = torch.zeros(16, dtype=torch.int32, device="cuda")
                assert L.vxrt_extract_surface(h, o3, d3, mode, work.data_ptr(), q.data_ptr() if cap else None, cap, None, None,
                                              summ.data_ptr(), None) == 0
                torch.cuda.synchronize()
                got = _summary(_u32(summ))
                print("checkerboard", mode, cap, got)
                assert got == want[:3] + (cap,) + want[4:], (mode, cap)
                q = _u32(q)
                assert np.array_equal(q[:2 * cap].reshape(-1, 2), thin.quads[:cap]) and (q[2 * cap:] == GUARD).all(), (mode, cap)
        del work
    finally:
        ctx.close()
        torch.cuda.empty_cache()


# ---- the denoiser
@pytest.fixture(scope="module")
def ctx(eng):
    vx, _ = eng
    c = new_ctx(vx)
    yield c
    c.close()


def _assert_filter(torch, ctx, c, keys, it, k, want, alias, what):
    """test_filter_equals_the_restatement's check of one call (tests/test_gpu_denoise.py)"""
    Hf, Wf = keys.shape
    n = Wf * Hf
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
    bad = RD.bits(got.cpu().numpy()) != RD.bits(want)
    print("denoise", what, "unequal", int(bad.sum()), np.argwhere(bad)[:3].tolist())
    assert not bad.any(), what
    assert np.array_equal(fb.cpu().numpy().reshape(Hf, Wf, 4), RD.bgra8(want)), what
    for whole in (cin_all, kk_all, out_all, fb_all, work_all):
        assert _guards_ok(torch, whole), what
    assert np.array_equal(kk.cpu().numpy().view(np.uint32).reshape(Hf, Wf), keys), what
    if alias:
        assert bool(torch.isnan(out).all()), what
    else:
        assert np.array_equal(RD.bits(cin.cpu().numpy().reshape(Hf, Wf, 3)), RD.bits(c)), what


@pytest.mark.parametrize("it", F.DN_ITERATIONS)
@pytest.mark.parametrize("k", F.DN_SCALES)
@pytest.mark.parametrize("Wf,Hf", F.THIN_FRAMES)
def test_frames_of_the_longest_side(eng, ctx, Wf, Hf, k, it):
    vx, torch = eng
    c, keys = RD.random_frame(Wf, Hf)
    assert ctx.denoise_workspace_bytes(Wf, Hf) == 32 * Wf * Hf and ctx.denoise_workspace_bytes(max(Wf, Hf) + 1, 1) == 0
    _assert_filter(torch, ctx, c, keys, it, k, F.denoised(Wf, Hf, k, it), (it + (k > 0)) % 2 == 1, (Wf, Hf, it, k))


@pytest.mark.parametrize("it", F.LIMIT_ITERATIONS)
@pytest.mark.parametrize("index", range(len(F.LIMIT_FRAMES)))
def test_frames_at_the_pixel_limit(eng, ctx, index, it):
    """the frame made of copies of a small random frame, the keys of every copy its own: the small frame's result, tiled"""
    vx, torch = eng
    (Wf, Hf), (tw, th) = F.LIMIT_FRAMES[index]
    tx, ty = Wf // tw, Hf // th
    n = Wf * Hf
    c, keys = RD.random_frame(tw, th)
    want = {k: F.denoised(tw, th, k, it) for k in F.DN_SCALES}
    assert ctx.denoise_workspace_bytes(Wf, Hf) == 32 * n > (1 << 31) - (1 << 23)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ids = (torch.arange(Hf, dtype=torch.int32, device="cuda") // th)[:, None] * tx + (torch.arange(Wf, dtype=torch.int32, device="cuda") // tw)[None, :] + 1
    kk, kk_all = _guarded(torch, n, torch.int32)
    small = dev(keys.view(np.int32)).repeat(ty, tx)
    kk.view(Hf, Wf).copy_(torch.where(small != 0, small ^ (ids << 8), small))
    del small, ids
    for row in (0, 1, ty - 1):  # the construction on the device is the module's
        assert np.array_equal(kk.view(Hf, Wf)[row * th:(row + 1) * th].cpu().numpy().view(np.uint32), F.tiled_keys_row(keys, tx, ty, row)), row
    ksum = int(kk.sum(dtype=torch.int64))
    big = dev(c).repeat(ty, tx, 1)
    cin, cin_all = _guarded(torch, 3 * n, torch.float32)
    out, out_all = _guarded(torch, 3 * n, torch.float32, float("nan"))
    fb, fb_all = _guarded(torch, 4 * n, torch.uint8, 7)
    work, work_all = _guarded(torch, 32 * n, torch.uint8, 0xA5)
    alias = index == F.LIMIT_ALIASED
    try:
        for k in F.DN_SCALES:
            cin.view(Hf, Wf, 3).copy_(big)
            src = cin.view(Hf, Wf, 3)
            got = ctx.denoise_frame(src, kk, it, k, out=src if alias else out.view(Hf, Wf, 3), fb=fb, work=work)
            torch.cuda.synchronize()
            expect = dev(RD.bits(want[k]).view(np.int32)).repeat(ty, tx, 1)
            bad = int((torch.where(torch.isnan(got), torch.full_like(expect, CANON), got.view(torch.int32)) != expect).sum())
            del expect
            pixels = dev(RD.bgra8(want[k]).view(np.int32).reshape(th, tw)).repeat(ty, tx)
            bad_fb = int((fb.view(torch.int32).view(Hf, Wf) != pixels).sum())
            del pixels
            print("pixel limit", (Wf, Hf), it, k, "unequal colours", bad, "pixels", bad_fb)
            assert bad == 0 and bad_fb == 0, (Wf, Hf, it, k)
            for whole in (cin_all, kk_all, out_all, fb_all, work_all):
                assert _guards_ok(torch, whole), (Wf, Hf, it, k)
            assert int(kk.sum(dtype=torch.int64)) == ksum  # (the keys' rows were compared above)
            if not alias:
                assert torch.equal(cin.view(torch.int32), big.view(-1).view(torch.int32))
    finally:
        del big, cin, cin_all, out, out_all, fb, fb_all, work, work_all, kk, kk_all
        torch.cuda.empty_cache()


def test_special_colours_and_scales(eng, ctx):
    vx, torch = eng
    c, keys, mask = F.special_frame()
    assert (mask & (keys != 0)).any() and (mask & (keys == 0)).any()
    for it in F.DN_ITERATIONS:
        for k in F.SPECIAL_SCALES:
            _assert_filter(torch, ctx, c, keys, it, k, RD.denoise_np(c, keys, it, k), False, ("special", it, k))


ORTHO_SIZE = (40.0, 30.0)


@pytest.fixture(scope="module")
def large_world(eng):
    """a context with the device-built 8192 x 512 x 8192 world: the keys read its extents, no table"""
    vx, _ = eng
    c = new_ctx(vx)
    c.SetOrthoWindowSize(*ORTHO_SIZE)
    c.build_world(vx.GEN_HASH_HEIGHTFIELD, *F.GUIDE_WORLD)
    yield c
    c.close()


@pytest.mark.parametrize("index", range(len(F.GUIDE_FRAMES)))
def test_guide_keys_of_a_world_of_2_35_voxels(eng, vxo, large_world, index):
    vx, torch = eng
    dims = F.GUIDE_WORLD[:3]
    total = dims[0] * dims[1] * dims[2]
    Wf, Hf = F.GUIDE_FRAMES[index]
    for ortho in (False, True):
        cam = helpers.camera("AD"[ortho], dims, vxo)
        hit = F.guide_hits(Wf, Hf, 2 * index + ortho)
        assert ((hit >= 1 << 32) & (hit < total)).sum() > 1000 and (hit >= total).sum() > 10 and (hit < 0).sum() > 10
        keys_all = torch.full((Hf * Wf + 64,), GUARD, dtype=torch.int32, device="cuda")
        keys = large_world.frame_guides(Wf, Hf, *cam, torch.from_numpy(hit).cuda(), ortho=ortho, out=keys_all)
        torch.cuda.synchronize()
        o, d = RD.primary_rays(Wf, Hf, *cam, ortho=ortho, ortho_size=ORTHO_SIZE)
        want = RD.keys_np(hit, dims, o, d)
        got = keys.cpu().numpy().view(np.uint32)
        bad = got != want
        print("keys", (Wf, Hf), ortho, "faces", len(np.unique(want)), "unequal", int(bad.sum()), hit[bad][:4].tolist())
        assert not bad.any(), (Wf, Hf, ortho)
        assert _guards_ok(torch, keys_all) and np.array_equal(got != 0, (hit >= 0) & (hit < total))
        assert len(np.unique(want >> 26)) > 2


def test_an_output_that_overlaps_the_input_in_part(eng, ctx):
    """d_color_out a row and a pixel above and below d_color_in, through the C call: the result of the restatement on the
    input as it was, the input outside the output and the words around both untouched"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    Wf, Hf = F.OVERLAP_FRAME
    n = Wf * Hf
    c, keys = RD.random_frame(Wf, Hf)
    flat = RD.bits(c).view(np.int32).reshape(-1)
    pad = 3 * Wf + 64
    kk = torch.from_numpy(keys.view(np.int32).reshape(-1).copy()).cuda()
    for it in F.OVERLAP_ITERATIONS:
        for k in F.DN_SCALES:
            want = RD.bits(RD.denoise_np(c, keys, it, k)).reshape(-1)
            for shift in F.overlap_shifts(Wf):
                s = shift // 4
                buf = torch.full((3 * n + 2 * pad,), GUARD, dtype=torch.int32, device="cuda")
                buf[pad:pad + 3 * n] = torch.from_numpy(c.reshape(-1).view(np.int32).copy()).cuda()
                work, work_all = _guarded(torch, 32 * n, torch.uint8, 0xA5)
                p = N.DenoiseParams(struct_size=C.sizeof(N.DenoiseParams), iterations=it, color_scale=k)
                cin = buf.data_ptr() + 4 * pad
                assert ctx._L.vxrt_denoise_frame(ctx._h, Wf, Hf, cin, kk.data_ptr(), C.byref(p), work.data_ptr(), cin + shift, None, None) == 0
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                out = RD.bits(got[pad + s:pad + s + 3 * n].view(np.float32)).view(np.uint32)
                what = (it, k, shift)
                print("overlap", what, "unequal", int((out != want).sum()))
                assert np.array_equal(out, want), what
                lo, hi = pad + min(s, 0), pad + 3 * n + max(s, 0)
                assert (got[:lo] == GUARD).all() and (got[hi:] == GUARD).all() and _guards_ok(torch, work_all), what
                kept = got[pad:pad + s] if s > 0 else got[pad + 3 * n + s:pad + 3 * n]
                assert np.array_equal(RD.bits(kept.view(np.float32)).view(np.int32), flat[:s] if s > 0 else flat[3 * n + s:]), what
