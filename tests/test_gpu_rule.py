"""Neighbour-count voxel rules on the device (include/vxrt.h, vxrt_apply_rule): the bits and the summary equal to
tests/ref_rule.py on gradient worlds at every brick edge, box width, neighbourhood, scope, iteration count and `outside`
value, with masks, on the hand-derived cases of tests/rule_cases.py, on every world path, after edits and stamps, through
smooth_voxels, on a bench-world window, on a box of more than 65 535 halo rows and at the ends of int32; determinism across
calls and streams; the host form; guard words; stream capture and replay; every refusal in the documented order, leaving the
outputs untouched; and the headless example's rule and smooth lines (which go through the facade)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region
from tests import ref_rule as R
from tests import rule_cases as RC
from tests.helpers import eng, gen_dense, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
WIDTHS = (1, 30, 31, 32, 33, 62, 63, 64, 65)
# every neighbourhood x scope x iteration count x `outside` value: 36 combinations, 12 per brick edge
COMBOS = [(nb, scope, n, outside) for n in (1, 2, 16) for scope in (R.BOX, R.WORLD) for nb in (R.N6, R.N18, R.N26) for outside in (0, 1)]
NONE = ((INT32_MAX,) * 3, (INT32_MIN,) * 3)


def _rule(vx, r: R.RefRule):
    return vx.Rule(r.neighbours, r.born, r.survive, r.iterations, r.scope, r.outside)


def _assert_rule(ctx, vx, world, origin, dims, rule, mask=None, stream=None, shift=(0, 0, 0)):
    """the device result against the reference computed on `world`, whose (0, 0, 0) is world voxel `shift`"""
    r = ctx.apply_rule(origin, dims, _rule(vx, rule), mask, stream=stream)
    want = R.apply_rule(world, tuple(int(a) - int(b) for a, b in zip(origin, shift)), dims, rule, mask)
    lo, hi = want["summary"][5:]
    if lo != NONE[0]:
        want["summary"] = (*want["summary"][:5], tuple(a + b for a, b in zip(lo, shift)), tuple(a + b for a, b in zip(hi, shift)))
    got = r.grid()
    print("rule", origin, dims, rule, tuple(r.summary), int((got != want["bits"]).sum()))
    assert np.array_equal(got, want["bits"]), (origin, dims, rule)
    assert tuple(r.summary) == want["summary"], (origin, dims, rule)
    return r, want


def _lively(rng, world, o, d, nb, scope, n, outside, mask=None):
    """random tables under which, by the reference, voxels of the box are born and die"""
    for _ in range(50):
        rule = R.random_rule(rng, nb, n, scope, outside)
        s = R.apply_rule(world, o, d, rule, mask)["summary"]
        if s[2] > 0 and s[3] > 0:
            return rule
    raise AssertionError("no lively rule for %r %r" % (o, d))


@pytest.mark.parametrize("index,factor,edge", [(0, 8, 64), (1, 16, 128), (2, 32, 256)])
def test_rule_equals_the_reference(eng, vxo, index, factor, edge):
    """dims[0] of 1, 30 .. 33 and 62 .. 65; origins negative, unaligned, over the far faces; the 36 combinations of
    neighbourhood, scope, iterations and `outside` spread over the three brick edges; every third BOX case with a mask"""
    vx, torch = eng
    rng = np.random.default_rng(factor)
    vox = R.gradient_world(rng, (edge, edge, edge))
    mid = edge // 2
    boxes = [((mid - 6, 3, 5), (WIDTHS[0], 9, 8)), ((-7, mid, -3), (WIDTHS[1], 6, 7)), ((edge - 20, edge - 4, 9), (WIDTHS[2], 7, 5)),
             ((11, -2, edge - 5), (WIDTHS[3], 5, 8)), ((-20, 17, mid), (WIDTHS[4], 6, 5)), ((edge - 50, 8, 1), (WIDTHS[5], 5, 6)),
             ((-3, mid + 1, mid - 1), (WIDTHS[6], 4, 7)), ((0, 0, 0), (WIDTHS[7], 6, 6)), ((edge - 33, edge - 3, edge - 3), (WIDTHS[8], 6, 6)),
             ((-5, -5, -5), (edge + 10, 12, 11)), ((mid - 9, mid - 8, mid - 7), (19, 18, 17)), ((3, 3, 3), (40, 5, 5))]
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, factor))
        for i, (o, d) in enumerate(boxes):
            nb, scope, n, outside = COMBOS[12 * index + i]
            mask = rng.random(d) < 0.8 if scope == R.BOX and i % 3 == 0 else None
            rule = _lively(rng, vox, o, d, nb, scope, n, outside, mask)
            _assert_rule(ctx, vx, vox, o, d, rule, mask)
        # wholly outside the world: nothing is free, the bits are 0 whatever `outside` says
        for o, d in [((edge + 3, 5, 5), (33, 4, 4)), ((5, -40, 5), (9, 20, 4))]:
            for outside in (0, 1):
                r, want = _assert_rule(ctx, vx, vox, o, d, R.random_rule(rng, R.N26, 2, outside, outside))
                assert tuple(r.summary) == (0, 0, 0, 0, 0, *NONE) and not r.grid().any()
    finally:
        ctx.close()


def test_every_table_entry_decides_some_voxel(eng, vxo):
    """the gradient cases of tests/rule_cases.py, in which every pair (self, count) decides some free voxel (asserted on the
    reference alone by tests/test_rule_host.py): every leaf of the two mux trees is looked up"""
    vx, torch = eng
    cases = RC.gradient_cases()
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(cases[0][0], 8))
        for w, o, d, rule, mask in cases:
            assert w is cases[0][0]
            r, want = _assert_rule(ctx, vx, w, o, d, rule, mask)
            assert want["summary"][2] > 0 and want["summary"][3] > 0
    finally:
        ctx.close()


def test_hand_derived_cases(eng, vxo):
    vx, torch = eng
    for case in RC.all_cases():
        ctx = vx.Context(0)
        try:
            upload(ctx, vxo.World.from_voxels(case["world"], 8))
            r = ctx.apply_rule(case["origin"], case["dims"], _rule(vx, case["rule"]), case["mask"])
            RC.check(case, {"bits": r.grid(), "summary": tuple(r.summary)}, r.bits.cpu().numpy())
            host = ctx.apply_rule_host(case["origin"], case["dims"], _rule(vx, case["rule"]), case["mask"])
            RC.check(case, {"bits": host.grid(), "summary": tuple(host.summary)})
        finally:
            ctx.close()


def _surface_box(vox, x0, x1, z0, z1, below, dims):
    heights = np.where(vox.any(1), vox.shape[1] - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
    return (x0, max(int(np.median(heights[max(x0, 0):x1, max(z0, 0):z1])) - below, 0), z0), dims


def test_every_world_path(eng, vxo, tmp_path):
    """a world built on the device, the same world saved and loaded into a second context, and its tables uploaded into a
    third: one rule, equal to the reference on the world read back"""
    vx, torch = eng
    a, b, c = vx.Context(0), vx.Context(0), vx.Context(0)
    try:
        a.build_world(vx.GEN_INT_TERRAIN, 256, 256, 256, 32)
        vox = a.read_region_host((0, 0, 0), (256, 256, 256))
        o, d = _surface_box(vox, -6, 94, 150, 256, 20, (100, 40, 120))
        rule = R.smooth(3, scope=R.WORLD)
        first, want = _assert_rule(a, vx, vox, o, d, rule)
        assert want["summary"][2] > 100 and want["summary"][3] > 100
        path = str(tmp_path / "w.vxb")
        a.save_world(path)
        b.load_world(path)
        w = a.download_world()
        c.upload_world(w["factor"], w["cdims"], w["coarse_bits"], w["brick_slot"], w["bounds"], w["pool"])
        for other in (b, c):
            r = other.apply_rule(o, d, _rule(vx, rule))
            assert torch.equal(r.bits, first.bits) and r.summary == first.summary
    finally:
        for ctx in (a, b, c):
            ctx.close()


def test_rule_follows_edits_and_stamps_and_smooth_voxels_writes_the_world(eng, vxo):
    """noise over a floor: the rule after an edit and after a stamp equals the reference on the restated world;
    smooth_voxels followed by read_region equals the restated world; BOX with n iterations equals n single calls with stamps"""
    vx, torch = eng
    rng = np.random.default_rng(4)
    vox = np.zeros((128, 128, 128), bool)
    vox[:, :20, :] = True
    vox[:, 20:60, :] = rng.random((128, 40, 128)) < 0.45
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (30, 10, -4), (60, 40, 50)
        rule = R.RefRule(R.N18, R.bits_of(range(8, 19)), R.bits_of(range(6, 19)), 2, R.BOX, 1)
        _assert_rule(ctx, vx, vox, o, d, rule)
        ops = [(1, 0, (60, 30, 20), (12, 0, 0)), (0, 1, (35, 25, 5), (50, 33, 9))]
        # no synchronisation between the edit and the rule: the call orders after the work queued on the stream
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        cur = ref_edit.apply_edits(vox, ops)
        _assert_rule(ctx, vx, cur, o, d, rule)
        stamps = [((56, 41, 6), rng.random((9, 7, 8)) < 0.5, vx.STAMP_REPLACE)]
        ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        cur = ref_region.apply_stamps(cur, stamps)
        res, want = _assert_rule(ctx, vx, cur, o, d, rule)
        # the result stamped: the world is the reference's
        ctx.edit_stamps([res.stamp()])
        cur = ref_region.apply_stamps(cur, [(o, want["bits"], vx.STAMP_REPLACE)])
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (128, 128, 128)), cur)
        # smooth_voxels with a mask, over the world's z-lo face
        mask = rng.random(d) < 0.7
        want = R.apply_rule(cur, o, d, R.smooth(2), mask)
        st, summary = ctx.smooth_voxels(o, d, 2, mask)
        assert tuple(summary) == want["summary"] and summary.born > 0 and summary.died > 0 and st.bricks_touched > 0
        cur = ref_region.apply_stamps(cur, [(o, want["bits"], vx.STAMP_REPLACE)])
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (128, 128, 128)), cur)
        # BOX, four iterations in one call = four calls of one iteration, each stamped
        rule4 = R.random_rule(rng, R.N26, 4, R.BOX, 0)
        whole, want4 = _assert_rule(ctx, vx, cur, o, d, rule4, mask)
        for _ in range(4):
            step = ctx.apply_rule(o, d, _rule(vx, rule4._replace(iterations=1)), mask)
            ctx.edit_stamps([step.stamp()])
        assert torch.equal(whole.bits, step.bits) and whole.summary.changed_last == step.summary.changed_last
        assert whole.summary.solid_after == step.summary.solid_after and whole.summary.born > 0 and whole.summary.died > 0
        assert np.array_equal(ctx.read_region_host(o, d), whole.grid()) and np.array_equal(whole.grid(), want4["bits"])
    finally:
        ctx.close()


def test_bench_world_window(eng):
    """a 256 x 128 x 256 window of the bench world at the terrain surface under Rule.smooth(2); the reference works on
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
        assert o[1] >= 1 and o[1] + d[1] + 1 <= 512  # the window and one voxel around it lie in the world: all of it is free
        shift = tuple(v - 1 for v in o)
        world = ctx.read_region_host(shift, tuple(v + 2 for v in d))  # voxel 0 at shift
        r, want = _assert_rule(ctx, vx, world, o, d, R.smooth(2), shift=shift)
        s = want["summary"]
        assert s[0] > 100000 and s[2] > 100 and s[3] > 100 and s[1] == s[0] + s[2] - s[3]
    finally:
        ctx.close()


def test_many_halo_rows_and_the_ends_of_int32(eng, vxo):
    """dims (1, 300, 300): 302 x 302 halo rows of one word, more rows than a grid axis of 65 535 would hold (the launch is 357
    workgroups on the first axis; tests/test_gpu_rule_frame_limits.py reaches the second); the last origins whose halo fits
    in int32, far from the world, with `outside` 0 and 1: nothing is free, the bits are 0; one voxel further is refused"""
    vx, torch = eng
    rng = np.random.default_rng(9)
    vox = R.gradient_world(rng, (128, 128, 128))
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        for scope, n in ((R.BOX, 2), (R.WORLD, 2)):
            o, d = (60, -90, -80), (1, 300, 300)
            _assert_rule(ctx, vx, vox, o, d, _lively(rng, vox, o, d, R.N26, scope, n, 1))
        d = (37, 9, 5)
        for scope, n, h in ((R.BOX, 3, 1), (R.WORLD, 16, 16)):
            for k in range(3):
                for edge, step in [(INT32_MIN + h, -1), (INT32_MAX - d[k] - h, 1)]:
                    for outside in (0, 1):
                        o = [300, 300, 300]
                        o[k] = edge
                        rule = vx.Rule.grow(vx.RULE_N26, n, scope=scope, outside=outside)
                        r = ctx.apply_rule(o, d, rule)
                        assert not bool(r.bits.any()) and tuple(r.summary) == (0, 0, 0, 0, 0, *NONE)
                        o[k] = edge + step
                        with pytest.raises(vx.VxrtError, match="beyond int32"):
                            ctx.apply_rule(o, d, rule)
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams_and_host_form(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(5)
    vox = R.gradient_world(rng, (128, 128, 128))
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (-5, 50, 7), (120, 40, 110)
        for nb, scope, n in ((R.N6, R.BOX, 2), (R.N18, R.WORLD, 3), (R.N26, R.WORLD, 16)):
            ref = _lively(rng, vox, o, d, nb, scope, n, 1)
            rule = _rule(vx, ref)
            mask = rng.random(d) < 0.6 if scope == R.BOX else None
            first = ctx.apply_rule(o, d, rule, mask)
            side = torch.cuda.Stream()
            for k in range(3):
                s = side.cuda_stream if k == 2 else None
                r = ctx.apply_rule(o, d, rule, mask, stream=s)
                if s is not None:
                    side.synchronize()
                assert r.summary == first.summary and torch.equal(r.bits, first.bits)
            host = ctx.apply_rule_host(o, d, rule, mask)
            assert np.array_equal(host.grid(), first.grid()) and host.summary == first.summary
            want = R.apply_rule(vox, o, d, ref, mask)
            assert tuple(first.summary) == want["summary"] and np.array_equal(first.grid(), want["bits"])
    finally:
        ctx.close()


def test_guard_words_behind_the_bits_the_summary_and_the_workspace(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(7)
    vox = R.gradient_world(rng)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        L, h = ctx._L, ctx._h
        i3 = lambda v: (C.c_int32 * 3)(*v)
        for (o, d), (nb, scope, n) in zip([((-3, 20, 5), (37, 21, 13)), ((30, 25, -1), (5, 7, 3)), ((0, 0, 0), (64, 64, 64))],
                                          [(R.N26, R.WORLD, 16), (R.N6, R.BOX, 2), (R.N18, R.WORLD, 1)]):
            ref = _lively(rng, vox, o, d, nb, scope, n, 0)
            rule = _rule(vx, ref)
            nw, ws = vx.region_words(d), ctx.rule_workspace_bytes(d, rule)
            work = torch.full((ws + 256,), 0xA5, dtype=torch.uint8, device="cuda")
            out = torch.full((nw + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            summ = torch.full((12 + 16,), 0x55555555, dtype=torch.int32, device="cuda")
            desc = rule._c()
            assert L.vxrt_apply_rule(h, i3(o), i3(d), C.byref(desc), None, work.data_ptr(), out.data_ptr(), summ.data_ptr(), None) == 0
            torch.cuda.synchronize()
            want = R.apply_rule(vox, o, d, ref)
            assert np.array_equal(vx.unpack_region(out[:nw], d), want["bits"])
            assert R.summary_from_words(summ[:12].cpu().numpy()) == want["summary"]
            assert bool((out[nw:] == 0x5A5A5A5A).all()) and bool((work[ws:] == 0xA5).all()) and bool((summ[12:] == 0x55555555).all())
            r = ctx.apply_rule(o, d, rule, out=out, work=work)  # the caller's buffers through the Python call
            assert np.array_equal(r.grid(), want["bits"]) and bool((out[nw:] == 0x5A5A5A5A).all())
    finally:
        ctx.close()


def test_a_captured_call_replays_on_the_world_as_it_is(eng, vxo):
    """vxrt_apply_rule captured into a graph on one side stream in torch's default capture mode and replayed over poisoned
    outputs: the reference on the world as uploaded, and after an edit inside the reserved pool the reference on the edited
    world"""
    vx, torch = eng
    from voxelengine_amd import _native as N
    rng = np.random.default_rng(3)
    vox = R.gradient_world(rng, (128, 128, 128))
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        ctx.edit_reserve((128 // 16) ** 3)
        capacity = ctx.edit_voxels([]).pool_capacity
        L, h = ctx._L, ctx._h
        i3 = lambda v: (C.c_int32 * 3)(*v)
        o, d = (-5, 40, 100), (70, 24, 37)  # over the world's x-lo and z-hi faces
        jobs = []
        for nb, scope, n, masked in ((R.N26, R.WORLD, 3, False), (R.N6, R.BOX, 2, True)):
            mask = rng.random(d) < 0.7 if masked else None
            ref = _lively(rng, vox, o, d, nb, scope, n, 1, mask)
            rule = _rule(vx, ref)
            jobs.append(dict(ref=ref, mask=mask, desc=rule._c(),
                             d_mask=None if mask is None else torch.from_numpy(vx.pack_region(mask).view(np.int32)).to("cuda"),
                             work=torch.zeros(ctx.rule_workspace_bytes(d, rule), dtype=torch.uint8, device="cuda"),
                             bits=torch.zeros(vx.region_words(d), dtype=torch.int32, device="cuda"),
                             summ=torch.zeros(12, dtype=torch.int32, device="cuda")))
        side = torch.cuda.Stream()

        def issue():
            for j in jobs:
                N.check(L.vxrt_apply_rule(h, i3(o), i3(d), C.byref(j["desc"]), None if j["d_mask"] is None else j["d_mask"].data_ptr(),
                                          j["work"].data_ptr(), j["bits"].data_ptr(), j["summ"].data_ptr(), side.cuda_stream))

        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            issue()

        def replay_and_check(world, tag):
            for _ in range(2):
                with torch.cuda.stream(side):
                    for j in jobs:
                        j["bits"].fill_(0x5A5A5A5A)
                        j["summ"].fill_(0x5A5A5A5A)
                        j["work"].fill_(0x5A)
                    g.replay()
                    side.synchronize()
                for j in jobs:
                    want = R.apply_rule(world, o, d, j["ref"], j["mask"])
                    assert np.array_equal(vx.unpack_region(j["bits"], d), want["bits"]), tag
                    assert R.summary_from_words(j["summ"].cpu().numpy()) == want["summary"], tag

        replay_and_check(vox, "as uploaded")
        ops = [(0, 0, (0, 0, 96), (15, 127, 127)), (0, 1, (3, 50, 105), (12, 58, 115)), (1, 0, (30, 50, 110), (6, 0, 0))]
        st = ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        assert st.pool_capacity == capacity  # nothing moved: the graph's addresses hold
        replay_and_check(ref_edit.apply_edits(vox, ops), "edited")
    finally:
        ctx.close()


def test_refusals_in_the_documented_order_leave_the_outputs_untouched(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        good = vx.Rule.smooth(2)
        ws = ctx.rule_workspace_bytes((8, 8, 8), vx.Rule.smooth(16, scope=vx.RULE_WORLD))
        assert ws > 0
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        out = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        summ = torch.full((12,), 0x55555555, dtype=torch.int32, device="cuda")
        mask = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        hmask = np.full(64, 0xFFFFFFFF, np.uint32)
        i3 = lambda *v: (C.c_int32 * 3)(*v)
        o3, d3 = i3(0, 0, 0), i3(8, 8, 8)
        hout, hsum = np.full(64, 0x5A5A5A5A, np.uint32), np.full(12, 0x55555555, np.uint32)

        def desc(**kw):
            r = good._c()
            for k, v in kw.items():
                setattr(r, k, v)
            return r

        def dev(o=o3, d=d3, r=None, m=False, wk=work.data_ptr(), ot=out.data_ptr(), s=summ.data_ptr()):
            r = desc() if r is None else r
            return L.vxrt_apply_rule(h, o, d, C.byref(r) if r != 0 else None, mask.data_ptr() if m else None, wk, ot, s, None)

        def host(o=o3, d=d3, r=None, m=False, ot=hout.ctypes.data, s=hsum.ctypes.data):
            r = desc() if r is None else r
            return L.vxrt_apply_rule_host(h, o, d, C.byref(r) if r != 0 else None, hmask.ctypes.data if m else None, ot, s)

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
        worst = dict(struct_size=28, neighbours=5, born=1 << 30, iterations=0, scope=7, outside=3, reserved_=1)
        for k in ("o", "d", "r", "wk", "ot", "s"):
            assert dev(**{"r": desc(**worst), "d": bad_d, k: 0 if k == "r" else None}) == -1, k
            assert "NULL argument" in L.vxrt_last_error().decode()
        for k in ("o", "d", "r", "ot", "s"):
            assert host(**{"r": desc(**worst), "d": bad_d, k: 0 if k == "r" else None}) == -1, k
            assert "NULL argument" in L.vxrt_last_error().decode()
        assert L.vxrt_apply_rule(None, o3, d3, C.byref(desc()), None, work.data_ptr(), out.data_ptr(), summ.data_ptr(), None) == -1
        order = [("struct_size", "size mismatch"), ("neighbours", "neighbours"), ("born", "a bit above"), ("iterations", "iterations"),
                 ("scope", "scope"), ("outside", "outside"), ("reserved_", "reserved_")]
        for i, (field, why) in enumerate(order):
            later = {k: worst[k] for k, _ in order[i:]}
            refused(why, r=desc(**later), m=True, d=bad_d, o=bad_o)
        for nb, n in ((vx.RULE_N6, 6), (vx.RULE_N18, 18), (vx.RULE_N26, 26)):
            refused("a bit above", r=desc(neighbours=nb, born=0, survive=2 << n))
            refused("a bit above", r=desc(neighbours=nb, born=2 << n, survive=0))
        for it in (0, -1, 17):
            refused("iterations", r=desc(iterations=it))
        refused("a mask with VXRT_RULE_WORLD", r=desc(scope=vx.RULE_WORLD), m=True, d=bad_d, o=bad_o)
        for bad in [(0, 8, 8), (8, -1, 8), (1024, 1024, 257)]:
            refused("box dims", d=i3(*bad), o=bad_o)
        refused("box dims", d=i3(1, 1, 1 << 28), r=desc(scope=vx.RULE_WORLD, iterations=16), o=bad_o)  # the halo box
        refused("beyond int32", o=bad_o)
        refused("beyond int32", o=i3(0, INT32_MIN, 0))
        refused("beyond int32", o=i3(0, INT32_MIN + 15, 0), r=desc(scope=vx.RULE_WORLD, iterations=16))
        assert dev(o=far_o) == -3 and host(m=True) == -3         # valid arguments: the missing world is next
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
        with pytest.raises(vx.VxrtError, match="a mask with VXRT_RULE_WORLD"):
            ctx.apply_rule((0, 0, 0), (8, 8, 8), vx.Rule.smooth(scope=vx.RULE_WORLD), np.ones((8, 8, 8), bool))
        assert dev() == 0 and host() == 0 and dev(o=far_o) == 0 and dev(m=True) == 0 and host(m=True) == 0
        assert dev(o=i3(0, INT32_MIN + 16, 0), r=desc(scope=vx.RULE_WORLD, iterations=16)) == 0
        torch.cuda.synchronize()
        assert not untouched()
    finally:
        ctx.close()


def test_headless_example_rule_and_smooth_lines(vxo, tmp_path):
    """examples/voxelapp_headless: a `rule` line (VoxelRaytracer3D::ApplyRule, then a stamp) and a `smooth` line
    (VoxelRaytracer3D::SmoothVoxels) on the same box; the printed summaries equal the reference's, the second on the world the
    first has left"""
    from oracle import vxo_edit
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    (ox, oy, oz), d = _surface_box(vox, 40, 140, -5, 65, 30, (100, 60, 70))
    hi = (ox + d[0] - 1, oy + d[1] - 1, oz + d[2] - 1)
    caves = R.RefRule(R.N18, R.bits_of(range(9, 19)), R.bits_of(range(7, 19)), 3, R.WORLD, 0)
    sf = tmp_path / "edits.txt"
    sf.write_text("0 rule %d %d %d %d %d %d n18 %x %x 3 world\n0 smooth %d %d %d %d %d %d 2\n"
                  % (ox, oy, oz, *hi, caves.born, caves.survive, ox, oy, oz, *hi))
    out = subprocess.run([exe, str(edge), "1", str(tmp_path / "rv"), "64", "48", "1", "-", "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    want, cur = [], vox
    for rule in (caves, R.smooth(2)):
        r = R.apply_rule(cur, (ox, oy, oz), d, rule)
        s = r["summary"]
        assert s[2] > 0 and s[3] > 0
        want.append("rule before frame 0: before %d after %d born %d died %d changed_last %d box %d %d %d %d %d %d," % (*s[:5], *s[5], *s[6]))
        cur = ref_region.apply_stamps(cur, [((ox, oy, oz), r["bits"], 0)])
    line = [x[:x.index(",") + 1] for x in out.stdout.splitlines() if x.startswith("rule before")]
    assert line == want, out.stdout
