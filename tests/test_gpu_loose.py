"""Loose voxels on the device (include/vxrt.h, vxrt_loose_step): the layer and the summary bit-equal to tests/ref_loose.py on
leaky-terrain worlds at every brick edge, box width, material, edge mode, step count and phase & 3, on boxes over every face
of the world, with material on every face of the box, on the hand-derived cases of tests/loose_cases.py, on every world path,
after edits and stamps, in place, split across calls, on a side stream, captured and replayed, through the host form and
settle_voxels, on a bench-world window and at the limits of the launches; guard words behind the output and the workspace;
every refusal in the documented order, leaving the outputs untouched; and the headless example's loose line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region
from tests import loose_cases as LC
from tests import ref_loose as R
from tests.helpers import eng, gen_dense, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
WIDTHS = (1, 31, 32, 33, 63, 64, 65)
STEPS = (1, 2, 5, 64)
NONE = R.NONE


def _params(vx, material, steps, edge, phase):
    return vx.Loose(material, steps, edge, phase)


def _assert_loose(ctx, vx, world, origin, dims, layer, material, steps, edge, phase, shift=(0, 0, 0), **kw):
    """the device result against the reference computed on `world`, whose (0, 0, 0) is world voxel `shift` (even offsets)"""
    r = ctx.loose_step(origin, dims, layer, _params(vx, material, steps, edge, phase), **kw)
    want = R.loose_step(world, tuple(int(a) - int(b) for a, b in zip(origin, shift)), dims, layer, material, steps, edge, phase)
    lo, hi = want["summary"][6:]
    if lo != NONE[0]:
        want["summary"] = (*want["summary"][:6], tuple(a + b for a, b in zip(lo, shift)), tuple(a + b for a, b in zip(hi, shift)))
    got = r.grid()
    print("loose", origin, dims, material, steps, edge, phase, tuple(r.summary), int((got != want["bits"]).sum()))
    assert np.array_equal(got, want["bits"]), (origin, dims, material, steps, edge, phase)
    assert tuple(r.summary) == want["summary"], (origin, dims, material, steps, edge, phase)
    return r, want


@pytest.mark.parametrize("index,factor,edge", [(0, 8, 64), (1, 16, 128), (2, 32, 256)])
def test_loose_equals_the_reference(eng, vxo, index, factor, edge):
    """box widths 1, 31 .. 33 and 63 .. 65 (halo rows that end at 3, 33 .. 35 and 65 .. 67 bits); origins negative, unaligned,
    over the far faces; both materials, both edges, 1, 2, 5 and 64 steps and every phase & 3 spread over the boxes and the
    three brick edges; dims 1 x 1 x 1, 1 x N x 1 and N x 1 x N"""
    vx, torch = eng
    rng = np.random.default_rng(factor)
    vox = R.terrain(rng, (edge, edge, edge), 1, 6, 0.15)
    boxes = [((edge // 2 - 6, 0, 5), (WIDTHS[0], 9, 8)), ((-7, 1, -3), (WIDTHS[1], 8, 7)), ((edge - 20, 0, 9), (WIDTHS[2], 9, 5)),
             ((11, -2, edge - 5), (WIDTHS[3], 9, 8)), ((-20, 2, edge // 2), (WIDTHS[4], 6, 5)), ((edge - 50, 0, 1), (WIDTHS[5], 7, 6)),
             ((-3, 1, edge // 2 - 1), (WIDTHS[6], 6, 7)), ((5, 3, 5), (1, 1, 1)), ((7, 0, 9), (1, 12, 1)), ((3, 4, 3), (40, 1, 37)),
             ((-5, -5, -5), (edge + 10, 14, 11)), ((0, 0, 0), (64, 10, 64))]
    ctx = vx.Context(0)
    moved = 0
    try:
        upload(ctx, vxo.World.from_voxels(vox, factor))
        for i, (o, d) in enumerate(boxes):
            k = i + index
            material, edge_mode, steps, phase = k & 1, (k >> 1) & 1, STEPS[(i + 2 * index) % 4], (5 * i + index) & 0xFFFFFFFF
            layer = R.random_layer(rng, d, 0.3)
            r, want = _assert_loose(ctx, vx, vox, o, d, layer, material, steps, edge_mode, phase)
            moved += sum(want["summary"][3:6])
        assert moved > 50
        # wholly outside the world: everything is dropped
        for o, d in [((edge + 3, 5, 5), (33, 4, 4)), ((5, -40, 5), (9, 20, 4))]:
            for edge_mode in (R.WALL, R.OPEN):
                layer = R.random_layer(rng, d, 0.5)
                r, want = _assert_loose(ctx, vx, vox, o, d, layer, R.WATER, 2, edge_mode, 1)
                assert tuple(r.summary)[1:6] == (0, 0, 0, 0, 0) and not r.grid().any() and r.summary.loose_in == int(layer.sum())
    finally:
        ctx.close()


def test_every_combination_on_one_box(eng, vxo):
    """both materials x both edges x steps 1, 2, 5, 64 x every phase & 3 on one box over the world's x-lo and y-lo faces"""
    vx, torch = eng
    rng = np.random.default_rng(17)
    vox = R.terrain(rng, (64, 64, 64), 1, 6, 0.15)
    o, d = (-3, -1, 20), (45, 12, 33)
    layer = R.random_layer(rng, d, 0.3)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        for material in (R.SAND, R.WATER):
            for edge_mode in (R.WALL, R.OPEN):
                for i, steps in enumerate(STEPS):
                    for phase in range(4):
                        if steps == 64 and phase != (material * 2 + edge_mode):
                            continue  # (64 steps of the reference take a second: one phase per material and edge)
                        _assert_loose(ctx, vx, vox, o, d, layer, material, steps, edge_mode, phase + 4 * i)
    finally:
        ctx.close()


def test_overhanging_boxes_and_material_on_every_face(eng, vxo):
    """boxes that overhang each face of the world (negative origins included), and a layer that is set on each of the six
    faces of the box in turn: under LOOSE_OPEN it drains through the faces that border empty space"""
    vx, torch = eng
    rng = np.random.default_rng(23)
    vox = R.terrain(rng, (64, 64, 64), 1, 4, 0.1)
    vox[:, 60:, :] |= rng.random((64, 4, 64)) < 0.3  # something solid at the world's top face
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        hang = [((-5, 2, 10), (20, 8, 9)), ((50, 2, 10), (20, 8, 9)), ((10, -4, 10), (9, 12, 9)), ((10, 55, 10), (9, 14, 9)),
                ((10, 2, -6), (9, 8, 20)), ((10, 2, 52), (9, 8, 20)), ((-2, -2, -2), (68, 68, 68))]
        for i, (o, d) in enumerate(hang):
            layer = R.random_layer(rng, d, 0.3 if d[0] < 60 else 0.02)
            for edge_mode in (R.WALL, R.OPEN):
                _assert_loose(ctx, vx, vox, o, d, layer, i & 1, 3, edge_mode, i)
        o, d = (20, 6, 20), (33, 7, 9)  # in mid-air: every face of the box borders empty space
        drained = 0
        for axis in range(3):
            for side in (0, -1):
                layer = np.zeros(d, bool)
                idx = [slice(None)] * 3
                idx[axis] = side
                layer[tuple(idx)] = True
                for material in (R.SAND, R.WATER):
                    for edge_mode in (R.WALL, R.OPEN):
                        r, want = _assert_loose(ctx, vx, vox, o, d, layer, material, 4, edge_mode, axis)
                        assert edge_mode == R.OPEN or want["summary"][2] == want["summary"][1]
                        drained += want["summary"][1] - want["summary"][2]
        assert drained > 100
    finally:
        ctx.close()


def test_hand_derived_cases_and_host_form(eng, vxo):
    vx, torch = eng
    worlds = {}
    try:
        for case in LC.hand_cases():
            key = case["world"].tobytes()
            if key not in worlds:
                worlds[key] = vx.Context(0)
                upload(worlds[key], vxo.World.from_voxels(case["world"], 8))
            ctx = worlds[key]
            p = _params(vx, case["material"], case["steps"], case["edge"], case["phase"])
            words = torch.from_numpy(LC.words_of(case).view(np.int32)).to("cuda")  # (with the padding bits the case sets)
            r = ctx.loose_step(case["origin"], case["dims"], words, p)
            LC.check(case, {"bits": r.grid(), "summary": tuple(r.summary)})
            host = ctx.loose_step_host(case["origin"], case["dims"], case["loose"], p)
            LC.check(case, {"bits": host.grid(), "summary": tuple(host.summary)})
    finally:
        for ctx in worlds.values():
            ctx.close()


def test_every_world_path(eng, vxo, tmp_path):
    """a world built on the device, the same world saved and loaded into a second context, and its tables uploaded into a
    third: one call, equal to the reference on the world read back"""
    vx, torch = eng
    a, b, c = vx.Context(0), vx.Context(0), vx.Context(0)
    try:
        a.build_world(vx.GEN_INT_TERRAIN, 256, 256, 256, 32)
        vox = a.read_region_host((0, 0, 0), (256, 256, 256))
        heights = np.where(vox.any(1), 255 - np.argmax(vox[:, ::-1, :], axis=1), 0)
        o, d = (-6, max(int(np.median(heights[:94, 150:])) - 10, 0), 150), (100, 40, 120)
        layer = R.random_layer(np.random.default_rng(1), d, 0.1)
        first, want = _assert_loose(a, vx, vox, o, d, layer, R.WATER, 6, R.OPEN, 2)
        assert sum(want["summary"][3:6]) > 100 and want["summary"][1] > 1000
        path = str(tmp_path / "w.vxb")
        a.save_world(path)
        b.load_world(path)
        w = a.download_world()
        c.upload_world(w["factor"], w["cdims"], w["coarse_bits"], w["brick_slot"], w["bounds"], w["pool"])
        for other in (b, c):
            r = other.loose_step(o, d, layer, _params(vx, R.WATER, 6, R.OPEN, 2))
            assert torch.equal(r.bits, first.bits) and r.summary == first.summary
    finally:
        for ctx in (a, b, c):
            ctx.close()


def _settle_ref(vox, o, d, so, sd, material, max_steps, edge):
    """settle_voxels restated: (the world afterwards, the last summary, the steps made)"""
    cur = vox.copy()
    src = tuple(slice(a, a + n) for a, n in zip(so, sd))
    layer = np.zeros(d, bool)
    layer[tuple(slice(a - b, a - b + n) for a, b, n in zip(so, o, sd))] = cur[src]
    cur[src] = False
    done = 0
    while done < max_steps:
        n = min(R.MAX_STEPS, max_steps - done)
        r = R.loose_step(cur, o, d, layer, material, n, edge, done)
        layer, done = r["bits"], done + n
        if r["summary"][3] + r["summary"][4] == 0:
            break
    return ref_region.apply_stamps(cur, [(o, layer, 1)]), r["summary"], done


def test_follows_edits_and_stamps_in_place_split_calls_and_settle_voxels(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(4)
    vox = R.terrain(rng, (128, 128, 128), 2, 9, 0.05)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (30, 0, -4), (60, 30, 50)
        layer = R.random_layer(rng, d, 0.15)
        _assert_loose(ctx, vx, vox, o, d, layer, R.SAND, 5, R.WALL, 0)
        ops = [(1, 0, (60, 5, 20), (8, 0, 0)), (0, 1, (35, 8, 5), (50, 9, 9))]
        # no synchronisation between the edit and the call: the call orders after the work queued on the stream
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        cur = ref_edit.apply_edits(vox, ops)
        _assert_loose(ctx, vx, cur, o, d, layer, R.WATER, 5, R.OPEN, 3)
        stamps = [((56, 6, 6), rng.random((9, 7, 8)) < 0.5, vx.STAMP_REPLACE)]
        ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        cur = ref_region.apply_stamps(cur, stamps)
        whole, want = _assert_loose(ctx, vx, cur, o, d, layer, R.WATER, 7, R.OPEN, 3)
        # in place equal to out of place
        words = torch.from_numpy(vx.pack_region(layer).view(np.int32)).to("cuda")
        inplace = ctx.loose_step(o, d, words, _params(vx, R.WATER, 7, R.OPEN, 3), out=words)
        assert inplace.bits.data_ptr() == words.data_ptr() and torch.equal(inplace.bits, whole.bits) and inplace.summary == whole.summary
        # split calls with the phase carried equal to one call
        cur_bits, first = torch.from_numpy(vx.pack_region(layer).view(np.int32)).to("cuda"), None
        for n, phase in ((3, 3), (1, 6), (3, 7)):
            step = ctx.loose_step(o, d, cur_bits, _params(vx, R.WATER, n, R.OPEN, phase), out=cur_bits)
            first = first or step.summary
        assert torch.equal(step.bits, whole.bits) and step.summary[2:6] == whole.summary[2:6] and first[:2] == whole.summary[:2]
        # the result stamped: the world is the reference's
        ctx.edit_stamps([whole.stamp()])
        cur = ref_region.apply_stamps(cur, [(o, want["bits"], vx.STAMP_UNION)])
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (128, 128, 128)), cur)
        # settle_voxels: a block of the terrain dug loose, both materials
        for material, edge_mode, max_steps in ((R.SAND, R.WALL, 200), (R.WATER, R.OPEN, 70)):
            bo, bd, so, sd = (20, 0, 60), (40, 24, 40), (30, 1, 70), (12, 8, 14)
            assert cur[tuple(slice(a, a + n) for a, n in zip(so, sd))].sum() > 50
            cur, ws, wn = _settle_ref(cur, bo, bd, so, sd, material, max_steps, edge_mode)
            summary, steps = ctx.settle_voxels(bo, bd, so, sd, material, max_steps, edge_mode)
            assert tuple(summary) == ws and steps == wn
            assert np.array_equal(ctx.read_region_host((0, 0, 0), (128, 128, 128)), cur)
        with pytest.raises(ValueError, match="inside"):
            ctx.settle_voxels((0, 0, 0), (8, 8, 8), (4, 4, 4), (8, 8, 8))
    finally:
        ctx.close()


def test_bench_world_window(eng):
    """a 256 x 128 x 256 window of the bench world at the terrain surface, 6 steps of water; the reference works on
    read_region_host of the window and one voxel around it"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz = 4000, 3000
        col = ctx.read_region_host((ox, 0, oz), (64, 512, 64))
        heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
        d = (256, 128, 256)
        o = (ox, min(max(int(np.median(heights)) - 64, 1), 511 - d[1]), oz)
        assert o[0] % 2 == 0 and o[1] >= 1 and o[1] + d[1] + 1 <= 512
        shift = (o[0] - 2, o[1] - 1 - (o[1] - 1) % 2, o[2] - 2)  # an even offset, so that the directions are the world's
        world = ctx.read_region_host(shift, tuple(v + 4 for v in d))  # voxel 0 at shift; covers the window and one voxel around
        rng = np.random.default_rng(2)
        layer = np.zeros(d, bool)
        layer[:, 96:104, :] = rng.random((256, 8, 256)) < 0.2
        # (the reference sees a world that ends where the read ends; under LOOSE_WALL what lies beyond the halo never matters)
        r, want = _assert_loose(ctx, vx, world, o, d, layer, R.WATER, 6, R.WALL, 0, shift=shift)
        s = want["summary"]
        assert s[1] > 50000 and s[2] == s[1] and s[5] > 100
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(5)
    vox = R.terrain(rng, (128, 128, 128), 1, 8, 0.1)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (-5, 0, 7), (120, 30, 110)
        layer = R.random_layer(rng, d, 0.2)
        for material, edge_mode, steps in ((R.SAND, R.WALL, 9), (R.WATER, R.OPEN, 6)):
            p = _params(vx, material, steps, edge_mode, 1)
            first, want = _assert_loose(ctx, vx, vox, o, d, layer, material, steps, edge_mode, 1)
            side = torch.cuda.Stream()
            for k in range(3):
                s = side.cuda_stream if k == 2 else None
                r = ctx.loose_step(o, d, layer, p, stream=s)
                if s is not None:
                    side.synchronize()
                assert r.summary == first.summary and torch.equal(r.bits, first.bits)
            host = ctx.loose_step_host(o, d, layer, p)
            assert np.array_equal(host.grid(), first.grid()) and host.summary == first.summary
    finally:
        ctx.close()


def test_guard_words_behind_the_layer_the_summary_and_the_workspace(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(7)
    vox = R.terrain(rng, (64, 64, 64), 1, 6, 0.15)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        L, h = ctx._L, ctx._h
        i3 = lambda v: (C.c_int32 * 3)(*v)
        for (o, d), (material, edge_mode, steps) in zip([((-3, 0, 5), (37, 21, 13)), ((30, 2, -1), (5, 7, 3)), ((0, 0, 0), (64, 64, 64))],
                                                       [(R.WATER, R.OPEN, 64), (R.SAND, R.WALL, 2), (R.WATER, R.WALL, 3)]):
            layer = R.random_layer(rng, d, 0.2)
            nw, ws = vx.region_words(d), ctx.loose_workspace_bytes(d)
            work = torch.full((ws + 256,), 0xA5, dtype=torch.uint8, device="cuda")
            out = torch.full((nw + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            inp = torch.full((nw + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            inp[:nw] = torch.from_numpy(vx.pack_region(layer).view(np.int32)).to("cuda")
            summ = torch.full((12 + 16,), 0x55555555, dtype=torch.int32, device="cuda")
            desc = _params(vx, material, steps, edge_mode, 2)._c()
            assert L.vxrt_loose_step(h, i3(o), i3(d), C.byref(desc), inp.data_ptr(), work.data_ptr(), out.data_ptr(), summ.data_ptr(), None) == 0
            torch.cuda.synchronize()
            want = R.loose_step(vox, o, d, layer, material, steps, edge_mode, 2)
            assert np.array_equal(vx.unpack_region(out[:nw], d), want["bits"])
            assert R.summary_from_words(summ[:12].cpu().numpy()) == want["summary"]
            assert bool((out[nw:] == 0x5A5A5A5A).all()) and bool((work[ws:] == 0xA5).all()) and bool((summ[12:] == 0x55555555).all())
            assert np.array_equal(vx.unpack_region(inp[:nw], d), layer) and bool((inp[nw:] == 0x5A5A5A5A).all())
            # in place through the C call: the guard words behind the one buffer hold
            assert L.vxrt_loose_step(h, i3(o), i3(d), C.byref(desc), inp.data_ptr(), work.data_ptr(), inp.data_ptr(), summ.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert torch.equal(inp[:nw], out[:nw]) and bool((inp[nw:] == 0x5A5A5A5A).all()) and bool((work[ws:] == 0xA5).all())
            r = ctx.loose_step(o, d, layer, _params(vx, material, steps, edge_mode, 2), out=out, work=work)  # the caller's buffers
            assert np.array_equal(r.grid(), want["bits"]) and bool((out[nw:] == 0x5A5A5A5A).all())
    finally:
        ctx.close()


def test_a_captured_call_replays_on_the_world_as_it_is(eng, vxo):
    """vxrt_loose_step captured into a graph on a side stream in global capture mode and replayed twice over poisoned outputs:
    the eager result; and after an edit inside the reserved pool the reference on the edited world"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    rng = np.random.default_rng(3)
    vox = R.terrain(rng, (128, 128, 128), 1, 8, 0.1)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        ctx.edit_reserve((128 // 16) ** 3)
        capacity = ctx.edit_voxels([]).pool_capacity
        L, h = ctx._L, ctx._h
        i3 = lambda v: (C.c_int32 * 3)(*v)
        o, d = (-5, 0, 100), (70, 24, 37)  # over the world's x-lo and z-hi faces
        jobs = []
        for material, edge_mode, steps in ((R.WATER, R.OPEN, 5), (R.SAND, R.WALL, 3)):
            layer = R.random_layer(rng, d, 0.2)
            jobs.append(dict(args=(material, steps, edge_mode, 1), layer=layer, desc=_params(vx, material, steps, edge_mode, 1)._c(),
                             inp=torch.from_numpy(vx.pack_region(layer).view(np.int32)).to("cuda"),
                             work=torch.zeros(ctx.loose_workspace_bytes(d), dtype=torch.uint8, device="cuda"),
                             bits=torch.zeros(vx.region_words(d), dtype=torch.int32, device="cuda"),
                             summ=torch.zeros(12, dtype=torch.int32, device="cuda")))
            jobs[-1]["eager"] = ctx.loose_step(o, d, layer, _params(vx, material, steps, edge_mode, 1))
        side = torch.cuda.Stream()

        def issue():
            for j in jobs:
                N.check(L.vxrt_loose_step(h, i3(o), i3(d), C.byref(j["desc"]), j["inp"].data_ptr(), j["work"].data_ptr(), j["bits"].data_ptr(),
                                          j["summ"].data_ptr(), side.cuda_stream))

        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side, capture_error_mode="global"):
            issue()

        def replay_and_check(world, tag, eager):
            for _ in range(2):
                with torch.cuda.stream(side):
                    for j in jobs:
                        j["bits"].fill_(0x5A5A5A5A)
                        j["summ"].fill_(0x5A5A5A5A)
                        j["work"].fill_(0x5A)
                    g.replay()
                    side.synchronize()
                for j in jobs:
                    want = R.loose_step(world, o, d, j["layer"], *j["args"])
                    assert np.array_equal(vx.unpack_region(j["bits"], d), want["bits"]), tag
                    assert R.summary_from_words(j["summ"].cpu().numpy()) == want["summary"], tag
                    if eager:
                        assert torch.equal(j["bits"], j["eager"].bits) and tuple(j["eager"].summary) == want["summary"]

        replay_and_check(vox, "as uploaded", True)
        ops = [(0, 0, (0, 0, 96), (15, 127, 127)), (0, 1, (3, 2, 105), (12, 8, 115)), (1, 0, (30, 3, 110), (6, 0, 0))]
        st = ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        assert st.pool_capacity == capacity  # nothing moved: the graph's addresses hold
        replay_and_check(ref_edit.apply_edits(vox, ops), "edited", False)
    finally:
        ctx.close()


def test_launch_limits(eng, vxo):
    """a box of exactly 2^28 voxels, one voxel high (16384 x 1 x 16384; the halo plane is 513 x 3 x 16386 words), loose material
    in patches whose windows the reference works on; one voxel more is refused; the last origins whose halo fits in int32, far
    from the world: everything is dropped, and one voxel further is refused; 64 steps of water (192 pass launches)"""
    vx, torch = eng
    rng = np.random.default_rng(9)
    vox = R.terrain(rng, (128, 128, 128), 1, 8, 0.1)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        n = 1 << 14
        o, d = (-4, 3, -6), (n, 1, n)
        assert d[0] * d[1] * d[2] == 1 << 28 and ctx.loose_workspace_bytes(d) > 0 and ctx.loose_workspace_bytes((n, 1, n + 1)) == 0
        nw = vx.region_words(d)
        wpr = n // 32
        words = torch.zeros(nw, dtype=torch.int32, device="cuda")
        # patches: over the world, at the far corner of the box, across a word boundary far out
        patches = [((2, 2), (140, 140)), ((n - 42, n - 42), (40, 40)), ((5000, 7000), (70, 9))]  # (two voxels off the box's faces)
        grids = []
        for (px, pz), (sx, sz) in patches:
            g = rng.random((sx, 1, sz)) < 0.4
            grids.append(g)
            full = np.zeros((sz, wpr * 32), bool)
            full[:, px:px + sx] = g[:, 0, :].T
            rows = torch.from_numpy(np.packbits(full, axis=-1, bitorder="little").view(np.int32).copy()).to("cuda")
            words.view(n, wpr)[pz:pz + sz] = rows
        total = sum(int(g.sum()) for g in grids)
        r = ctx.loose_step(o, d, words, _params(vx, R.WATER, 2, R.WALL, 0))
        s = r.summary
        out = r.bits.view(n, wpr)
        # the box is one voxel high and walled: nothing falls or slides, water spreads within its one layer by at most one voxel
        # a step, so a window two voxels around a patch holds all of it; outside the world everything is dropped
        in_world = 0
        for ((px, pz), (sx, sz)), g in zip(patches, grids):
            po = (o[0] + px - 2, o[1], o[2] + pz - 2)
            pd = (sx + 4, 1, sz + 4)
            layer = np.zeros(pd, bool)
            layer[2:-2, :, 2:-2] = g
            want = R.loose_step(vox, po, pd, layer, R.WATER, 2, R.WALL, 0)
            got_rows = out[pz - 2:pz + sz + 2].cpu().numpy().view(np.uint32)
            bits = np.unpackbits(got_rows.view(np.uint8), axis=-1, bitorder="little").astype(bool)
            got, ref = bits[:, px - 2:px + sx + 2].T, want["bits"][:, 0, :]
            assert np.array_equal(got, ref), (px, pz)
            in_world += want["summary"][1]
        assert int(r.bits.ne(0).sum()) > 0 and s.loose_in == total and s.loose_start == in_world == s.loose_after and s.spread_last > 0
        assert s.fell_last == 0 and s.slid_last == 0
        del words, r, out
        d = (37, 9, 5)
        for k in range(3):
            for edge, step in [(INT32_MIN + 1, -1), (INT32_MAX - d[k] - 1, 1)]:
                for edge_mode in (R.WALL, R.OPEN):
                    og = [300, 300, 300]
                    og[k] = edge
                    layer = R.random_layer(rng, d, 0.5)
                    r = ctx.loose_step(og, d, layer, _params(vx, R.WATER, 3, edge_mode, 0))
                    lo = tuple(og[a] + int(np.argwhere(layer)[:, a].min()) for a in range(3))
                    hi = tuple(og[a] + int(np.argwhere(layer)[:, a].max()) for a in range(3))
                    assert not bool(r.bits.any()) and tuple(r.summary) == (int(layer.sum()), 0, 0, 0, 0, 0, lo, hi)
                    og[k] = edge + step
                    with pytest.raises(vx.VxrtError, match="beyond int32"):
                        ctx.loose_step(og, d, layer, _params(vx, R.WATER, 3, edge_mode, 0))
        # 64 steps of water: the most launches a call makes
        o, d = (10, 0, 10), (100, 20, 100)
        _assert_loose(ctx, vx, vox, o, d, R.random_layer(rng, d, 0.1), R.WATER, 64, R.OPEN, 0xFFFFFFF0)
        with pytest.raises(vx.VxrtError, match="steps"):
            ctx.loose_step(o, d, np.zeros(d, bool), _params(vx, R.WATER, 65, R.OPEN, 0))
    finally:
        ctx.close()


def test_refusals_in_the_documented_order_leave_the_outputs_untouched(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        ws = ctx.loose_workspace_bytes((8, 8, 8))
        assert ws > 0
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        out = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        summ = torch.full((12,), 0x55555555, dtype=torch.int32, device="cuda")
        inp = torch.full((64,), 0x01010101, dtype=torch.int32, device="cuda")
        hin = np.full(64, 0x01010101, np.uint32)
        i3 = lambda *v: (C.c_int32 * 3)(*v)
        o3, d3 = i3(0, 0, 0), i3(8, 8, 8)
        hout, hsum = np.full(64, 0x5A5A5A5A, np.uint32), np.full(12, 0x55555555, np.uint32)

        def desc(**kw):
            p = vx.Loose(vx.LOOSE_WATER, 2, vx.LOOSE_OPEN, 1)._c()
            for k, v in kw.items():
                if k == "reserved_":
                    p.reserved_[1] = v
                else:
                    setattr(p, k, v)
            return p

        def dev(o=o3, d=d3, p=None, li=inp.data_ptr(), wk=work.data_ptr(), ot=out.data_ptr(), s=summ.data_ptr()):
            p = desc() if p is None else p
            return L.vxrt_loose_step(h, o, d, C.byref(p) if p != 0 else None, li, wk, ot, s, None)

        def host(o=o3, d=d3, p=None, li=hin.ctypes.data, ot=hout.ctypes.data, s=hsum.ctypes.data):
            p = desc() if p is None else p
            return L.vxrt_loose_step_host(h, o, d, C.byref(p) if p != 0 else None, li, ot, s)

        def untouched():
            torch.cuda.synchronize()
            return (bool((out == 0x5A5A5A5A).all()) and bool((summ == 0x55555555).all()) and (hout == 0x5A5A5A5A).all()
                    and (hsum == 0x55555555).all())

        def refused(why, **kw):
            """both forms refuse with VXRT_ERR_INVALID and the message of the check `why`"""
            for call in (dev, host):
                assert call(**kw) == -1, kw
                assert why in L.vxrt_last_error().decode(), (why, L.vxrt_last_error())

        bad_d, bad_o, far_o = i3(0, 8, 8), i3(INT32_MAX - 8, 0, 0), i3(INT32_MAX - 9, 0, 0)
        assert dev() == -3 and host() == -3 and untouched()    # no world
        # each check comes before every later one, and before the missing world
        worst = dict(struct_size=28, material=5, steps=0, edge=7, reserved_=1)
        for k in ("o", "d", "p", "li", "wk", "ot", "s"):
            assert dev(**{"p": desc(**worst), "d": bad_d, k: 0 if k == "p" else None}) == -1, k
            assert "NULL argument" in L.vxrt_last_error().decode()
        for k in ("o", "d", "p", "li", "ot", "s"):
            assert host(**{"p": desc(**worst), "d": bad_d, k: 0 if k == "p" else None}) == -1, k
            assert "NULL argument" in L.vxrt_last_error().decode()
        assert L.vxrt_loose_step(None, o3, d3, C.byref(desc()), inp.data_ptr(), work.data_ptr(), out.data_ptr(), summ.data_ptr(), None) == -1
        order = [("struct_size", "size mismatch"), ("material", "material"), ("steps", "steps"), ("edge", "edge"), ("reserved_", "reserved_")]
        for i, (field, why) in enumerate(order):
            later = {k: worst[k] for k, _ in order[i:]}
            refused(why, p=desc(**later), d=bad_d, o=bad_o)
        for steps in (0, -1, 65):
            refused("steps", p=desc(steps=steps))
        for bad in [(0, 8, 8), (8, -1, 8), (1024, 1024, 257)]:
            refused("box dims", d=i3(*bad), o=bad_o)
        refused("beyond int32", o=bad_o)
        refused("beyond int32", o=i3(0, INT32_MIN, 0))
        assert dev(o=far_o) == -3 and host() == -3         # valid arguments: the missing world is next
        assert untouched()
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        refused("beyond int32", o=bad_o)
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        refused("streamed")
        ctx.stream_close()
        assert untouched()
        ctx.load_world(path)
        assert dev() == 0 and host() == 0 and dev(o=far_o) == 0 and dev(o=i3(0, INT32_MIN + 1, 0)) == 0
        torch.cuda.synchronize()
        assert not untouched()
    finally:
        ctx.close()


def test_headless_example_loose_line(vxo, tmp_path):
    """examples/voxelapp_headless: two `loose` lines (VoxelRaytracer3D::SettleVoxels without the early stop, which goes through
    StepLoose), sand walled and then water open on the world the first has left; the printed summaries equal the reference's"""
    from oracle import vxo_edit
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    heights = np.where(vox.any(1), edge - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
    top = int(np.median(heights[40:140, :65]))
    o, d = (40, max(top - 30, 0), -5), (100, 60, 70)
    so, sd = (70, max(top - 12, 0), 10), (30, 14, 30)
    hi = tuple(a + n - 1 for a, n in zip(o, d))
    shi = tuple(a + n - 1 for a, n in zip(so, sd))
    lines = [("sand", "wall", R.SAND, R.WALL, 70), ("water", "open", R.WATER, R.OPEN, 9)]
    sf = tmp_path / "edits.txt"
    sf.write_text("".join("0 loose %s %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n" % (m, *o, *hi, *so, *shi, steps, e)
                          for m, e, _, _, steps in lines))
    out = subprocess.run([exe, str(edge), "1", str(tmp_path / "rv"), "64", "48", "1", "-", "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    want, cur = [], vox
    for _, _, material, edge_mode, steps in lines:
        src = tuple(slice(a, a + n) for a, n in zip(so, sd))
        layer = np.zeros(d, bool)
        layer[tuple(slice(a - b, a - b + n) for a, b, n in zip(so, o, sd))] = cur[src]
        assert layer.sum() > 100
        cur = cur.copy()
        cur[src] = False
        done = 0
        while done < steps:
            n = min(R.MAX_STEPS, steps - done)
            r = R.loose_step(cur, o, d, layer, material, n, edge_mode, done)
            layer, done = r["bits"], done + n
        s = r["summary"]
        want.append("loose before frame 0: in %d start %d after %d fell_last %d slid_last %d spread_last %d box %d %d %d %d %d %d,"
                    % (*s[:6], *s[6], *s[7]))
        cur = ref_region.apply_stamps(cur, [(o, layer, 1)])
    line = [x[:x.index(",") + 1] for x in out.stdout.splitlines() if x.startswith("loose before")]
    assert line == want, out.stdout
