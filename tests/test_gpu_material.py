"""The voxel materials on the device (include/vxrt.h, vxrt_material_field / vxrt_material_frame).  Field: bytes and summary
bit-equal to tests/ref_material.py on the boxes of tests/material_cases.py (widths 1 .. 257, heights across y segments and the
warm-up, boxes over every face of the world) at every brick edge, with and without paint, into aligned and unaligned outputs,
with guard bytes.  Frame: colours, BGRA8, ids and summary bit-equal on the frames of the host tests, with every optional
output present and absent, tile edges 1, 8 and 64, without an atlas, with a tile withheld, the output aliasing the input, guard
bytes.  Consistency with no restatement involved (the ids of a rendered frame are the field's bytes; the field passed back as
paint changes nothing); every world path; edits and stamps; a bench-world window; the ends of int32; a side stream; capture and
replay; determinism; every refusal in the documented order; the headless example's materials line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import material_cases as MC
from tests import ref_denoise as R
from tests import ref_material as M
from tests.helpers import eng, gen_dense, new_ctx, upload
from tests.test_gpu_denoise import WORLDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GUARD_BYTES = 256
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
_CACHE = {}


def _rules(vx, rules=MC.RULES):
    return vx.MaterialRules(tuple(rules))


def _palette(vx, n_tiles=5, shift=3, with_atlas=True):
    tints, tiles = MC.palette(n_tiles)
    return vx.Palette(tints, tiles, MC.atlas(n_tiles, shift) if with_atlas else None)


def _guarded(torch, a=None, nbytes=0, fill=0x7B, lead=0):
    """a device byte tensor holding the numpy array `a` (or `nbytes` bytes of `fill`) `lead` bytes in, with GUARD_BYTES bytes of
    0x5A behind it (and 0x5A in the lead)"""
    raw = np.full(nbytes, fill, np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.full((lead + raw.size + GUARD_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    t[lead:lead + raw.size].copy_(torch.from_numpy(raw.copy()))
    return t


def _payload(t, dtype, shape, lead=0):
    return t[lead:t.numel() - GUARD_BYTES].cpu().numpy().view(dtype).reshape(shape)


def _want_field(i, paint=True):
    key = ("field", i, paint)
    if key not in _CACHE:
        origin, dims = MC.FIELD_BOXES[i]
        _CACHE[key] = M.material_field_np(MC.terrain_world(), origin, dims, MC.RULES, MC.paint_bytes() if paint else None, MC.PAINT_BOX)
    return _CACHE[key]


def _want_frame(Wf, Hf, ortho, pose, **kw):
    key = ("frame", Wf, Hf, ortho, pose, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = MC.run_frame(MC.frame_case(Wf, Hf, ortho, pose), **kw)[:3]
    return _CACHE[key]


def _summary(words):
    return (int(words[0]), int(words[1]), int(words[2]), [int(v) for v in words[4:260]])


# ---- the field against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", (8, 16, 32))
def test_the_field_equals_the_restatement(eng, vxo, factor):
    """through the C ABI, the output and the summary with guard bytes behind them: with paint into a 4-byte aligned output (one
    dword per lane and row where the width is a multiple of four), without paint into an output one to three bytes off"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    edge = 8 * factor
    world = np.zeros((edge, edge, edge), bool)
    world[:64, :64, :64] = MC.terrain_world()
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(world, factor))
        d_paint = _guarded(torch, MC.paint_bytes().transpose(2, 1, 0))
        for i, (origin, dims) in enumerate(MC.FIELD_BOXES):
            n = dims[0] * dims[1] * dims[2]
            for paint, lead in ((True, 0), (False, 1 + i % 3)):
                want = _want_field(i, paint)
                d_out, d_sum = _guarded(torch, nbytes=n, lead=lead), _guarded(torch, nbytes=1040)
                r = _rules(vx)._c(MC.PAINT_BOX)
                rc = L.vxrt_material_field(ctx._h, (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims), C.byref(r),
                                           d_paint.data_ptr() if paint else None, d_out.data_ptr() + lead, d_sum.data_ptr(), None)
                assert rc == 0, L.vxrt_last_error()
                torch.cuda.synchronize()
                what = (factor, origin, dims, paint, lead)
                got = _payload(d_out, np.uint8, dims[::-1], lead).transpose(2, 1, 0)
                assert np.array_equal(got, want[0]), what
                assert _summary(_payload(d_sum, np.uint32, (260,))) == want[1] and _payload(d_sum, np.uint32, (260,))[3] == 0, what
                for t in (d_out, d_sum, d_paint):
                    assert bool((t[-GUARD_BYTES:] == 0x5A).all()), what
                assert bool((d_out[:lead] == 0x5A).all()), what
        assert np.array_equal(_payload(d_paint, np.uint8, MC.PAINT_BOX[1][::-1]), MC.paint_bytes().transpose(2, 1, 0))
    finally:
        ctx.close()


def test_the_hand_derived_columns(eng, vxo):
    """the three-layer column with paint (50, 0, 60), and the overhang, through the Python mirror and the host call"""
    vx, torch = eng
    w = np.zeros(MC.WORLD, bool)
    w[4, 3:10, 4] = True
    w[9, 0:6, 9] = True
    w[9, 10:12, 9] = True
    three = vx.MaterialRules(((None, 1, 2, 3, 2),))
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(w, 8))
        paint = np.array([50, 0, 60], np.uint8).reshape(1, 3, 1)
        for f in (ctx.material_field((4, 0, 4), (1, 12, 1), three, paint, ((4, 7, 4), (1, 3, 1))),
                  ctx.material_field_host((4, 0, 4), (1, 12, 1), three, paint, ((4, 7, 4), (1, 3, 1)))):
            assert f.grid()[0, :, 0].tolist() == [0, 0, 0, 3, 3, 3, 3, 50, 2, 60, 0, 0]
            s = f.summary
            assert (s.solid, s.painted, s.top) == (7, 2, 1) and s.hist[0] == 5 and s.hist[3] == 4 and s.hist[50] == 1
        f = ctx.material_field((9, 0, 9), (1, 13, 1), three)
        assert f.grid()[0, :, 0].tolist() == [3, 3, 3, 2, 2, 1, 0, 0, 0, 0, 2, 1, 0] and f.summary.top == 2
    finally:
        ctx.close()


# ---- the frame against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wf,Hf,ortho,pose", MC.FRAME_CASES)
def test_the_frame_equals_the_restatement(eng, vxo, Wf, Hf, ortho, pose):
    """through the C ABI, every buffer with guard bytes behind it: every output; the colour output aliasing the input; no
    framebuffer, ids or summary, and each of the three alone; no atlas and no paint; tiles of one texel; tiles of 64 x 64 with the last tile withheld"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    case = MC.frame_case(Wf, Hf, ortho, pose)
    n = Wf * Hf
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(case["world"], 8))
        ctx.SetOrthoWindowSize(*case["ortho_size"])
        modes = [("all", {}), ("alias", {}), ("bare", {}), ("fb", {}), ("ids", {}), ("sum", {}), ("plain", dict(with_atlas=False, paint=False)), ("T1", dict(shift=0, n_tiles=1)),
                 ("T64", dict(shift=6, n_tiles=3, told_tiles=2))]
        for mode, kw in modes:
            color, ids, summary = _want_frame(Wf, Hf, ortho, pose, **kw)
            shift, n_tiles = kw.get("shift", 3), kw.get("n_tiles", 5)
            pal = _palette(vx, n_tiles, shift, kw.get("with_atlas", True))
            paint = kw.get("paint", True)
            d_col, d_keys, d_hit = _guarded(torch, case["color"]), _guarded(torch, case["keys"]), _guarded(torch, case["hit"])
            d_paint, d_pal = _guarded(torch, MC.paint_bytes().transpose(2, 1, 0)), _guarded(torch, pal.entries())
            d_atl = _guarded(torch, pal.atlas_words()) if pal.atlas is not None else None
            d_out, d_fb, d_ids, d_sum = _guarded(torch, nbytes=12 * n), _guarded(torch, nbytes=4 * n), _guarded(torch, nbytes=n), _guarded(torch, nbytes=16)
            given = {"bare": (), "fb": ("fb",), "ids": ("ids",), "sum": ("sum",)}.get(mode, ("fb", "ids", "sum"))  # the optional outputs
            out = d_col if mode == "alias" else d_out
            r = _rules(vx)._c(MC.PAINT_BOX)
            p = N.MaterialFrameParams(struct_size=C.sizeof(N.MaterialFrameParams), ortho=int(ortho), n_tiles=kw.get("told_tiles", pal.n_tiles),
                                      tile_shift=shift)
            p.cam.origin, p.cam.fwd, p.cam.up, p.cam.right = ((C.c_float * 3)(*[float(x) for x in v]) for v in case["cam"])
            rc = L.vxrt_material_frame(ctx._h, Wf, Hf, d_col.data_ptr(), d_keys.data_ptr(), d_hit.data_ptr(), C.byref(r),
                                       d_paint.data_ptr() if paint else None, d_pal.data_ptr(), d_atl.data_ptr() if d_atl is not None else None,
                                       C.byref(p), out.data_ptr(), d_fb.data_ptr() if "fb" in given else None,
                                       d_ids.data_ptr() if "ids" in given else None, d_sum.data_ptr() if "sum" in given else None, None)
            assert rc == 0, L.vxrt_last_error()
            torch.cuda.synchronize()
            what = (Wf, Hf, ortho, pose, mode)
            assert np.array_equal(R.bits(_payload(out, F32, (Hf, Wf, 3))), R.bits(color)), what
            for name, t in (("fb", d_fb), ("ids", d_ids), ("sum", d_sum)):
                if name not in given:
                    assert bool((t[:-GUARD_BYTES] == 0x7B).all()), what
            if "fb" in given:
                assert np.array_equal(_payload(d_fb, np.uint8, (Hf, Wf, 4)), R.bgra8(color)), what
            if "ids" in given:
                assert np.array_equal(_payload(d_ids, np.uint8, (Hf, Wf)), ids), what
            if "sum" in given:
                assert tuple(_payload(d_sum, np.uint32, (4,)).tolist()) == summary, what
            for t in [d_col, d_keys, d_hit, d_paint, d_pal, d_out, d_fb, d_ids, d_sum] + ([d_atl] if d_atl is not None else []):
                assert bool((t[-GUARD_BYTES:] == 0x5A).all()), what
            assert np.array_equal(_payload(d_keys, np.uint32, (Hf, Wf)), case["keys"]) and np.array_equal(_payload(d_hit, np.int64, (Hf, Wf)), case["hit"]), what
            if mode == "alias":
                assert bool((d_out[:-GUARD_BYTES] == 0x7B).all()), what
            else:
                assert np.array_equal(R.bits(_payload(d_col, F32, (Hf, Wf, 3))), R.bits(case["color"])), what
    finally:
        ctx.close()


# ---- consistency on rendered frames, no restatement involved ---------------------------------------------------------------
W, H = 160, 96


def _render(vx, torch, ctx, cam, stream=None):
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.full((H, W), -7, dtype=torch.int64, device="cuda")
    ctx.RenderScreen(W, H, fb, *cam, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=3), color_aov=col, hit_aov=hit, stream=stream)
    keys = ctx.frame_guides(W, H, *cam, hit, stream=stream)
    return col, keys, hit, fb


@pytest.mark.parametrize("factor", sorted(WORLDS))
def test_the_ids_of_a_rendered_frame_are_the_fields_bytes_and_the_field_as_paint_changes_nothing(eng, vxo, factor):
    vx, torch = eng
    X, Y, Z = dims = WORLDS[factor]
    rules = vx.MaterialRules(((None, 1, 2, 3, 3), (Y // 2, 4, 5, 6, 0), (Y * 3 // 4, 7, 8, 9, 15)))
    pal = _palette(vx)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z), X, Y, Z, factor))
        cam = helpers.camera("A", dims, vxo)
        col, keys, hit, fb = _render(vx, torch, ctx, cam)
        got = ctx.material_frame(col, keys, hit, cam, rules, pal, fb=fb, material_aov=True)
        box = ((X // 4, 0, Z // 8), (X // 2, Y, Z // 2))  # part of the world: some hits inside it, some outside
        field = ctx.material_field(*box, rules)
        whole = ctx.material_field((0, 0, 0), dims, rules).grid()
        h = hit.cpu().numpy()
        ids = got.materials.cpu().numpy()
        hm = h >= 0
        v = (h[hm] % X, h[hm] // X % Y, h[hm] // (X * Y))
        assert hm.sum() > W * H // 5 and np.array_equal(ids[hm], whole[v]) and not ids[~hm].any() and ids[hm].min() >= 1
        assert len(np.unique(ids[hm])) >= 3
        s = got.summary
        assert s.hit == int(hm.sum()) and s.painted == 0 and 0 < s.top <= s.hit and 0 < s.textured < s.hit
        assert np.array_equal(fb.cpu().numpy(), R.bgra8(got.color.cpu().numpy()))
        assert not np.array_equal(R.bits(got.color.cpu().numpy()), R.bits(col.cpu().numpy()))
        again = ctx.material_frame(col, keys, hit, cam, rules, pal, paint=field, material_aov=True)
        assert torch.equal(again.color.view(torch.int32), got.color.view(torch.int32)) and torch.equal(again.materials, got.materials)
        inside = np.ones(int(hm.sum()), bool)
        for k in range(3):
            inside &= (v[k] >= box[0][k]) & (v[k] < box[0][k] + box[1][k])
        a = again.summary
        assert 0 < inside.sum() < hm.sum() and a.painted == int(inside.sum()) and (a.hit, a.top, a.textured) == (s.hit, s.top, s.textured)
    finally:
        ctx.close()


def test_every_world_path(eng, vxo, tmp_path):
    """a world built on the device, the same world saved and loaded into a second context, and its tables uploaded into a
    third: one field and one frame, the field equal to the restatement on the world read back"""
    vx, torch = eng
    a, b, c = new_ctx(vx), new_ctx(vx), new_ctx(vx)
    rules = vx.MaterialRules(((None, 1, 2, 3, 3), (120, 7, 8, 9, 15)))
    try:
        a.build_world(vx.GEN_INT_TERRAIN, 256, 256, 256, 32)
        o, d = (-6, 60, 150), (100, 110, 57)
        sub = a.read_region_host((o[0], o[1], o[2]), (d[0], 256 - o[1], d[2]))  # the box's columns up to the world's top
        shifted = [(None if r[0] is None else r[0] - o[1], *r[1:]) for r in rules.bands]
        want = M.material_field_np(sub, (0, 0, 0), d, shifted)
        first = a.material_field(o, d, rules)
        assert np.array_equal(first.grid(), want[0]) and _summary(first._words()) == want[1] and want[1][0] > 10000 and want[1][2] > 1000
        path = str(tmp_path / "w.vxb")
        a.save_world(path)
        b.load_world(path)
        w = a.download_world()
        c.upload_world(w["factor"], w["cdims"], w["coarse_bits"], w["brick_slot"], w["bounds"], w["pool"])
        cam = helpers.camera("A", (256, 256, 256), vxo)
        frames = []
        for ctx in (a, b, c):
            r = ctx.material_field(o, d, rules)
            assert np.array_equal(r.grid(), first.grid()) and r.summary == first.summary
            col, keys, hit, _ = _render(vx, torch, ctx, cam)
            frames.append(ctx.material_frame(col, keys, hit, cam, rules, _palette(vx), material_aov=True))
        for f in frames[1:]:
            assert torch.equal(f.color.view(torch.int32), frames[0].color.view(torch.int32)) and torch.equal(f.materials, frames[0].materials)
            assert f.summary == frames[0].summary and f.summary.hit > 1000
    finally:
        for ctx in (a, b, c):
            ctx.close()


def test_the_field_follows_edits_and_stamps(eng, vxo):
    """solid ground up to y = 39 under one band (1, 2, 3, depth 2): the voxels at y = 30 are `deep`.  An edit digs a shaft down
    to y = 31: the shaft's floor at y = 30 becomes `top`, y = 29 and 28 `under`.  A stamp puts a lid over the shaft at y = 35:
    the floor has air above it still -- `top` -- the lid over the shaft is `top`, and the ground beside the shaft is as it was."""
    vx, torch = eng
    vox = np.zeros((128, 128, 128), bool)
    vox[:, :40, :] = True
    rules = vx.MaterialRules(((None, 1, 2, 3, 2),))
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (50, 20, 50), (20, 30, 20)
        before = ctx.material_field(o, d, rules).grid()
        assert before[10, 10, 10] == 3 and before[10, 19, 10] == 1 and before[10, 18, 10] == 2
        ctx.edit_voxels([vx.EditBox((58, 31, 58), (61, 60, 61), 0)])  # no synchronisation: the field orders after the edit
        vox[58:62, 31:61, 58:62] = False
        dug = ctx.material_field(o, d, rules)
        want = M.material_field_np(vox, o, d, rules.bands)
        assert np.array_equal(dug.grid(), want[0]) and _summary(dug._words()) == want[1]
        assert dug.grid()[10, 10, 10] == 1 and dug.grid()[10, 9, 10] == 2 and dug.grid()[10, 7, 10] == 3 and dug.grid()[10, 11, 10] == 0
        ctx.edit_stamps([vx.Stamp((56, 35, 56), np.ones((8, 1, 8), bool), vx.STAMP_UNION)])
        vox[56:64, 35, 56:64] = True
        lid = ctx.material_field(o, d, rules)
        want = M.material_field_np(vox, o, d, rules.bands)
        assert np.array_equal(lid.grid(), want[0]) and _summary(lid._words()) == want[1]
        assert lid.grid()[10, 10, 10] == 1 and lid.grid()[10, 15, 10] == 1 and lid.grid()[10, 14, 10] == 0 and np.array_equal(lid.grid()[7], before[7])
    finally:
        ctx.close()


def test_bench_world_window(eng):
    """a 257 x 140 x 9 window of the bench world across the terrain surface: the restatement works on read_region_host of the
    window's columns up to the world's top"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz = 4000, 3000
        col = ctx.read_region_host((ox, 0, oz), (64, 512, 64))
        heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
        o, d = (ox - 3, max(int(np.median(heights)) - 100, 0), oz + 5), (257, 140, 9)
        sub = ctx.read_region_host(o, (d[0], 512 - o[1], d[2]))
        bands = ((None, 1, 2, 3, 3), (o[1] + 90, 7, 8, 9, 15))
        want = M.material_field_np(sub, (0, 0, 0), d, [(None if r[0] is None else r[0] - o[1], *r[1:]) for r in bands])
        got = ctx.material_field(o, d, vx.MaterialRules(bands))
        assert np.array_equal(got.grid(), want[0]) and _summary(got._words()) == want[1]
        assert want[1][0] > 10000 and want[1][2] > 500 and want[1][3][0] > 10000
    finally:
        ctx.close()


def test_boxes_at_the_ends_of_int32(eng, vxo):
    """the first and the last origin the contract allows, far from the world: every byte 0; one voxel further is refused.
    A paint box at the ends of int32 is looked up and never hit."""
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        d = (37, 9, 5)
        n = d[0] * d[1] * d[2]
        rules = _rules(vx)
        paint = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
        for k in range(3):
            for edge, step in [(INT32_MIN, None), (INT32_MAX - d[k] - 16, 1)]:
                o = [300, 300, 300]
                o[k] = edge
                f = ctx.material_field(o, d, rules, paint, ((INT32_MAX - d[0], INT32_MAX - d[1], INT32_MAX - d[2]), d))
                s = f.summary
                assert not f.grid().any() and (s.solid, s.painted, s.top) == (0, 0, 0) and s.hist[0] == n and sum(s.hist) == n
                if step:
                    o[k] = edge + step
                    with pytest.raises(vx.VxrtError):
                        ctx.material_field(o, d, rules)
        # a box that reaches from far below the world into it, and paint whose box starts at the least int32
        o, dd = (10, -70, 10), (5, 100, 3)
        f = ctx.material_field(o, dd, rules, torch.full((4 * 200 * 3,), 99, dtype=torch.uint8, device="cuda"), ((INT32_MIN, -100, 9), (4, 200, 3)))
        assert not f.grid()[:, :70, :].any() and f.summary.painted == 0 and f.summary.solid > 0
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams_and_the_host_form(eng, vxo):
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(MC.terrain_world(), 8))
        o, d = MC.FIELD_BOXES[8]
        rules = _rules(vx)
        paint = torch.from_numpy(np.ascontiguousarray(MC.paint_bytes().transpose(2, 1, 0))).cuda()
        first = ctx.material_field(o, d, rules, paint, MC.PAINT_BOX)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for k in range(3):
            s = side.cuda_stream if k == 2 else None
            r = ctx.material_field(o, d, rules, paint, MC.PAINT_BOX, stream=s)
            if s is not None:
                side.synchronize()
            assert r.summary == first.summary and torch.equal(r.materials, first.materials)
        host = ctx.material_field_host(o, d, rules, MC.paint_bytes(), MC.PAINT_BOX)
        assert np.array_equal(host.grid(), first.grid()) and host.summary == first.summary
        want = M.material_field_np(MC.terrain_world(), o, d, MC.RULES, MC.paint_bytes(), MC.PAINT_BOX)
        assert np.array_equal(first.grid(), want[0]) and _summary(first._words()) == want[1]
        # the frame: twice on the current stream, once on a side stream
        case = MC.frame_case(96, 64, False, "up")
        ctx.SetOrthoWindowSize(*case["ortho_size"])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        args = (dev(case["color"]), dev(case["keys"].view(np.int32)), dev(case["hit"]), case["cam"], rules, _palette(vx))
        want = _want_frame(96, 64, False, "up")
        torch.cuda.synchronize()
        for k in range(3):
            s = side.cuda_stream if k == 2 else None
            with torch.cuda.stream(side) if s is not None else torch.cuda.stream(torch.cuda.current_stream()):
                g = ctx.material_frame(*args, paint=paint, paint_box=MC.PAINT_BOX, material_aov=True, stream=s)
            if s is not None:
                side.synchronize()
            assert tuple(g.summary) == want[2]
            assert np.array_equal(R.bits(g.color.cpu().numpy()), R.bits(want[0])) and np.array_equal(g.materials.cpu().numpy(), want[1])
    finally:
        ctx.close()


def test_capture_and_replay_over_poisoned_outputs(eng, vxo):
    """both device calls captured in global mode on a side stream and replayed twice over outputs filled with other values"""
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(MC.terrain_world(), 8))
        rules, pal = _rules(vx), _palette(vx)
        o, d = MC.FIELD_BOXES[3]
        n = d[0] * d[1] * d[2]
        case = MC.frame_case(65, 9, False, "up")
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        col, keys, hit = dev(case["color"]), dev(case["keys"].view(np.int32)), dev(case["hit"])
        paint = dev(MC.paint_bytes().transpose(2, 1, 0))
        eager_field = ctx.material_field(o, d, rules, paint, MC.PAINT_BOX)
        eager = ctx.material_frame(col, keys, hit, case["cam"], rules, pal, paint=paint, paint_box=MC.PAINT_BOX, material_aov=True)
        torch.cuda.synchronize()
        want = _want_frame(65, 9, False, "up")
        assert np.array_equal(R.bits(eager.color.cpu().numpy()), R.bits(want[0])) and tuple(eager.summary) == want[2]
        out_f = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        out_c = torch.full_like(col, 7.0)
        out_fb = torch.full((9, 65, 4), 0xEE, dtype=torch.uint8, device="cuda")
        out_ids = torch.full((9, 65), 0xEE, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rf = ctx.material_field(o, d, rules, paint, MC.PAINT_BOX, out=out_f)
            rc = ctx.material_frame(col, keys, hit, case["cam"], rules, pal, paint=paint, paint_box=MC.PAINT_BOX, out=out_c, fb=out_fb,
                                    material_aov=out_ids)
        assert bool((out_f == 0xEE).all()) and bool((out_c == 7.0).all())  # capturing ran nothing
        for _ in range(2):
            out_f.fill_(0xEE)
            out_c.fill_(7.0)
            out_fb.fill_(0xEE)
            out_ids.fill_(0xEE)
            rf._summary.fill_(77)
            rc._summary.fill_(77)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                g.replay()
            side.synchronize()
            assert torch.equal(out_f, eager_field.materials) and [int(x) for x in rf._summary.cpu()] == eager_field._words()
            assert torch.equal(out_c.view(torch.int32), eager.color.view(torch.int32)) and torch.equal(out_ids, eager.materials)
            assert np.array_equal(out_fb.cpu().numpy(), R.bgra8(want[0])) and tuple(int(x) for x in rc._summary.cpu()) == tuple(eager.summary)
    finally:
        ctx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order_with_nothing_written(eng, vxo, tmp_path):
    vx, torch = eng
    from voxelengine_amd import _native as N
    L = N.load()
    n = 16 * 8
    col = torch.full((8, 16, 3), 0.5, dtype=torch.float32, device="cuda")
    keys = torch.full((n,), 0x1234, dtype=torch.int32, device="cuda")
    hit = torch.full((n,), 1, dtype=torch.int64, device="cuda")  # voxel (1, 0, 0): inside the paint box
    paint = torch.full((64,), 0x33, dtype=torch.uint8, device="cuda")
    pal = torch.zeros((256 * 5,), dtype=torch.int32, device="cuda")
    out = torch.full((8, 16, 3), 9.0, dtype=torch.float32, device="cuda")
    fb = torch.full((n,), 0x1234, dtype=torch.int32, device="cuda")
    ids = torch.full((n,), 0x12, dtype=torch.uint8, device="cuda")
    summary = torch.full((4,), 0x1234, dtype=torch.int32, device="cuda")
    mats = torch.full((64,), 0x12, dtype=torch.uint8, device="cuda")
    fsum = torch.full((260,), 0x1234, dtype=torch.int32, device="cuda")
    nan, inf = float("nan"), float("inf")
    empty, streamed, world = vx.Context(0), vx.Context(0), new_ctx(vx)
    GOOD = ((None, 1, 2, 3, 3), (20, 4, 5, 6, 0))

    def err():
        return L.vxrt_last_error().decode()

    def rules_c(rsize=None, n_bands=None, bands=GOOD, rreserved=0, pdims=(4, 4, 4), porigin=(0, 0, 0)):
        r = vx.MaterialRules(tuple(bands))._c((porigin, pdims))
        if rsize is not None:
            r.struct_size = rsize
        if n_bands is not None:
            r.n_bands = n_bands
        r.reserved_ = rreserved
        return r

    def frame(h=empty._h, Wf=16, Hf=8, size=C.sizeof(N.MaterialFrameParams), params=True, n_tiles=0, shift=3, reserved=0, bad=None, rules=True,
              cp=col.data_ptr(), kp=keys.data_ptr(), hp=hit.data_ptr(), pp=pal.data_ptr(), op=out.data_ptr(), paintp=paint.data_ptr(), **rk):
        p = N.MaterialFrameParams(struct_size=size, ortho=0, n_tiles=n_tiles, tile_shift=shift, reserved_=reserved)
        p.cam.origin, p.cam.fwd, p.cam.up, p.cam.right = ((C.c_float * 3)(*v) for v in ((1, 2, 3), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
        if bad:
            field, k, v = bad
            getattr(p.cam, field)[k] = v
        r = rules_c(**rk)
        return L.vxrt_material_frame(h, Wf, Hf, cp, kp, hp, C.byref(r) if rules else None, paintp, pp, None, C.byref(p) if params else None, op,
                                     fb.data_ptr(), ids.data_ptr(), summary.data_ptr(), None)

    def field(h=empty._h, origin=(0, 0, 0), dims=(4, 4, 4), rules=True, op=True, dp=True, mp=mats.data_ptr(), sp=fsum.data_ptr(),
              paintp=paint.data_ptr(), **rk):
        r = rules_c(**rk)
        return L.vxrt_material_field(h, (C.c_int32 * 3)(*origin) if op else None, (C.c_int32 * 3)(*dims) if dp else None,
                                     C.byref(r) if rules else None, paintp, mp, sp, None)

    try:
        # the frame: each call has the earlier faults mended and all the later ones still in it; the context holds no world
        later = dict(size=8, n_tiles=4097, n_bands=9, bad=("fwd", 1, nan), pdims=(0, 4, 4), cp=None)
        assert frame(h=None, Wf=0, **later) == -1 and "ctx" in err()
        for Wf, Hf in ((0, 8), (16, 0), (65536, 1), (1, 65536), (8193, 8192)):
            assert frame(Wf=Wf, Hf=Hf, **later) == -1 and "W, H" in err()
        assert frame(**later) == -1 and "vxrt_material_frame_params" in err()
        later.pop("size")
        assert frame(params=False, cp=None) == -1 and "vxrt_material_frame_params" in err()
        for kw in (dict(n_tiles=4097), dict(n_tiles=0, shift=7), dict(n_tiles=0, reserved=1)):
            assert frame(**dict(later, **kw)) == -1 and "n_tiles" in err()
        later.pop("n_tiles")
        assert frame(**dict(later, rules=False)) == -1 and "vxrt_material_rules" in err()
        assert frame(**dict(later, rsize=96)) == -1 and "vxrt_material_rules" in err()
        for nb in (0, 9):
            assert frame(**dict(later, n_bands=nb)) == -1 and "n_bands" in err()
        later.pop("n_bands")
        for bands in (((5, 1, 2, 3, 3),), ((None, 1, 2, 3, 3), (-(1 << 31), 4, 5, 6, 0)), ((None, 0, 2, 3, 3),), ((None, 1, 0, 3, 3),),
                      ((None, 1, 2, 0, 3),), ((None, 1, 2, 3, 16),), ((None, 1, 2, 3, 3), (7, 1, 1, 1, 1), (7, 1, 1, 1, 1))):
            assert frame(**dict(later, bands=bands)) == -1 and "bands[0]" in err(), bands
        assert frame(**dict(later, rreserved=1)) == -1 and "reserved_" in err()  # the rules' reserved_ comes before the pose
        for fld in ("origin", "fwd", "up", "right"):
            for k, v in ((0, nan), (2, inf), (1, -inf)):
                assert frame(**dict(later, bad=(fld, k, v))) == -1 and "non-finite" in err()
        later.pop("bad")
        for kw in (dict(pdims=(0, 4, 4)), dict(pdims=(4, -1, 4)), dict(pdims=(1 << 10, 1 << 10, (1 << 8) + 1)), dict(pdims=(4, 4, 4), porigin=(0, 2 ** 31 - 4, 0))):
            assert frame(**dict(later, **kw)) == -1 and "paint box" in err()
        assert frame(**dict(later, paintp=None)) == -1 and "NULL" in err()  # without paint the box is not looked at
        later.pop("pdims")
        for kw in (dict(cp=None), dict(kp=None), dict(hp=None), dict(pp=None), dict(op=None)):
            assert frame(**kw) == -1 and "NULL" in err()
        assert frame() == -3 and "no world" in err()  # VXRT_ERR_NO_WORLD

        # the field
        fl = dict(n_bands=9, pdims=(0, 4, 4), dims=(0, 4, 4), origin=(0, INT32_MAX - 10, 0))
        for kw in (dict(h=None), dict(op=False), dict(dp=False), dict(rules=False), dict(mp=None), dict(sp=None)):
            assert field(**dict(fl, **kw)) == -1 and "NULL" in err()
        assert field(**dict(fl, rsize=104)) == -1 and "vxrt_material_rules" in err()
        assert field(**fl) == -1 and "n_bands" in err()
        fl.pop("n_bands")
        assert field(**dict(fl, bands=((None, 1, 2, 3, 16),))) == -1 and "bands[0]" in err()
        assert field(**dict(fl, rreserved=2)) == -1 and "reserved_" in err()
        assert field(**fl) == -1 and "paint box" in err()
        fl.pop("pdims")
        assert field(**fl) == -1 and "box dims" in err()
        assert field(**dict(fl, paintp=None, pdims=(0, 0, 0))) == -1 and "box dims" in err()
        for dims in ((4, -1, 4), (1 << 10, 1 << 10, (1 << 8) + 1)):
            assert field(**dict(fl, dims=dims)) == -1 and "box dims" in err()
        fl.pop("dims")
        assert field(**fl) == -1 and "origin" in err()
        assert field(origin=(0, INT32_MAX - 4 - 15, 0)) == -1 and "origin" in err()
        assert field(origin=(0, INT32_MAX - 4 - 16, 0)) == -3 and "no world" in err()
        assert field() == -3 and "no world" in err()

        # a streamed world is a cache: it is not queried
        w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16)
        upload(world, w)
        path = str(tmp_path / "w.vxb")
        world.save_world(path)
        streamed.stream_open(path, 1000)
        assert frame(h=streamed._h) == -1 and "streamed" in err()
        assert field(h=streamed._h) == -1 and "streamed" in err()
        torch.cuda.synchronize()
        assert bool((out == 9.0).all()) and bool((ids == 0x12).all()) and bool((fb == 0x1234).all()) and bool((summary == 0x1234).all())
        assert bool((mats == 0x12).all()) and bool((fsum == 0x1234).all())
        assert bool((col == 0.5).all()) and bool((keys == 0x1234).all()) and bool((hit == 1).all()) and bool((paint == 0x33).all())
        # and the same arguments on a resident world are accepted
        assert frame(h=world._h) == 0 and field(h=world._h) == 0
        torch.cuda.synchronize()
        assert summary.tolist()[0] == n and not bool((out == 9.0).any()) and not bool((fb == 0x1234).any()) and bool((ids == 0x33).all())
        assert int(fsum[4:].sum()) == 64 and not bool((mats == 0x12).any())
    finally:
        for c in (empty, streamed, world):
            c.close()


# ---- the example ---------------------------------------------------------------------------------------------------------
def _example_palette(vx):
    pal = vx.Palette()
    for m in range(1, 6):
        pal.set(m, top=m - 1)
    pal.set(1, top=0, side=5, bottom=1)
    base = np.array([(80, 180, 60), (134, 96, 67), (128, 128, 128), (220, 205, 140), (245, 245, 255), (110, 140, 70)], np.uint64)
    t, r, s = np.meshgrid(np.arange(6, dtype=np.uint64), np.arange(8, dtype=np.uint64), np.arange(8, dtype=np.uint64), indexing="ij")
    m32 = np.uint64(0xFFFFFFFF)
    n = (((((t * np.uint64(73856093)) & m32) ^ ((r * np.uint64(19349663)) & m32) ^ ((s * np.uint64(83492791)) & m32)) * np.uint64(2654435761)) & m32) >> np.uint64(24)
    shade = np.uint64(192) + (n >> np.uint64(2))
    atlas = np.full((6, 8, 8, 4), 255, np.uint8)
    atlas[..., :3] = (base[:, None, None, :] * shade[..., None] // np.uint64(255)).astype(np.uint8)
    return vx.Palette(pal.tints, pal.tiles, atlas)


def test_headless_example_materials_line(eng, vxo, tmp_path):
    """examples/voxelapp_headless on a path of three poses with "0 materials" and "2 materials off": the summary lines of frames
    0 and 1 are those of the Python path on the same world, the dumped PPMs the coloured frames, and frame 2 is the plain
    frame"""
    vx, torch = eng
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge, Wf, Hf = 256, 64, 48
    f32 = lambda v: tuple(float(F32(x)) for x in v)
    eulers = [f32((-0.45 + 0.005 * j, 0.7 + 0.01 * j, 0.0)) for j in range(3)]
    positions = [f32((edge * 0.25 + 0.5 * j, edge * 0.9 - 0.25 * j, edge * 0.25 + 0.25 * j)) for j in range(3)]
    (tmp_path / "path.txt").write_text("".join("%r %r %r %r %r %r\n" % (*p, *e) for p, e in zip(positions, eulers)))
    (tmp_path / "script.txt").write_text("0 materials\n2 materials off\n")
    out = subprocess.run([exe, str(edge), "3", str(tmp_path / "mf"), str(Wf), str(Hf), "2", str(tmp_path / "path.txt"), "1", "1", "1",
                          "0x0x0", str(tmp_path / "script.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [x for x in out.stdout.splitlines() if x.startswith("materials ")]
    assert len(lines) == 2, out.stdout
    rules = vx.MaterialRules(((None, 1, 2, 3, 3), (edge // 8 * 5, 5, 4, 3, 1)))
    pal = _example_palette(vx)
    dense = gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(dense, edge, edge, edge, 32))
        coloured = 0
        for j in range(3):
            f, u, r = vxo.get_directions(eulers[j])
            cam = (positions[j], f, u, r)
            fb = torch.zeros((Hf, Wf, 4), dtype=torch.uint8, device="cuda")
            col = torch.zeros((Hf, Wf, 3), dtype=torch.float32, device="cuda")
            hit = torch.zeros((Hf, Wf), dtype=torch.int64, device="cuda")
            ctx.RenderScreen(Wf, Hf, fb, *cam, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=j), color_aov=col, hit_aov=hit)
            if j < 2:
                keys = ctx.frame_guides(Wf, Hf, *cam, hit)
                got = ctx.material_frame(col, keys, hit, cam, rules, pal, fb=fb)
                s = got.summary
                assert lines[j] == "materials frame %d hit %d painted %d top %d textured %d" % (j, *s), (j, lines)
                assert s.hit > 100 and s.textured == s.hit and s.painted == 0
            torch.cuda.synchronize()
            ppm = open(tmp_path / ("mf_%04d.ppm" % j), "rb").read()
            rgb = np.frombuffer(ppm[-Wf * Hf * 3:], np.uint8).reshape(Hf, Wf, 3)
            assert np.array_equal(rgb, fb.cpu().numpy()[..., 2::-1]), j
            coloured += int((rgb.max(-1).astype(int) - rgb.min(-1) > 8).sum()) if j < 2 else 0
        assert coloured > 200  # the frames are no longer grey
    finally:
        ctx.close()
