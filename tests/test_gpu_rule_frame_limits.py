"""Voxel rules, reprojection and the light on frames on the device at the limits of their launches: the cases of
tests/rule_frame_limit_cases.py, each bit for bit against tests/ref_rule.py, tests/ref_reproject.py or
tests/ref_light_frame.py, or against an identity that tests/test_rule_frame_limits_host.py holds against them: rule planes of
2^20 + 1 workgroups on the second grid axis with a workspace past 2^32 bytes, rows of 2^23 words, the output launch in its
middle branch and at its cap, the summary's counters at 2^28, worlds of three different sides under the rule and under the
light on frames, frames of 65535 pixels a side and a frame of nearly 2^26 pixels in the counted and the plain launch of both
frame kernels, NaN, infinite, negative-zero and denormal operands, the light on frames on the 8192 x 512 x 8192 bench world
(hit indices past 2^32) and with light boxes of 2^28 bytes and at x = -2^31.  The large results are compared on the device;
the large outputs and workspaces have guard words behind them."""
import numpy as np
import pytest

from tests import ref_denoise as RD
from tests import ref_reproject as T
from tests import light_frame_cases as LC
from tests import rule_frame_limit_cases as F
from tests import helpers
from tests import ref_light_frame as LF
from tests.helpers import eng, new_ctx, upload
from tests.read_limit_cases import checker_stamp_rows, pack_region, small_world
from tests.test_gpu_reproject import _guarded, _guards_ok

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
PATTERN = 0x7FC12345  # a NaN with a payload: no output holds it
F32 = np.float32


def _rule(vx, r):
    return vx.Rule(r.neighbours, r.born, r.survive, r.iterations, r.scope, r.outside)


def _ctx(vx, vxo, vox, factor):
    ctx = vx.Context(0)
    upload(ctx, vxo.World.from_voxels(np.asarray(vox), factor))
    return ctx


def _guarded_rule(torch, ctx, vx, o, d, rule, layout):
    """the call with a poisoned workspace and a poisoned output, guard bytes behind both: (the output's words, the summary)"""
    ws = ctx.rule_workspace_bytes(d, _rule(vx, rule))
    assert ws == layout.total
    work = torch.full((ws + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((layout.nb + 64,), GUARD, dtype=torch.int32, device="cuda")
    r = ctx.apply_rule(o, d, _rule(vx, rule), out=out, work=work)
    summary = tuple(r.summary)
    torch.cuda.synchronize()
    assert r.bits.data_ptr() == out.data_ptr() and r.bits.numel() == layout.nb
    assert bool((out[layout.nb:] == GUARD).all()) and bool((work[ws:] == 0xA5).all())
    del work
    return out[:layout.nb], summary


# ---- rules
@pytest.mark.parametrize("outside", (0, 1))
@pytest.mark.parametrize("k", (0, 1))
def test_rule_planes_on_the_second_grid_axis(eng, vxo, k, outside):
    """case 1: 2^20 + 1 workgroups of plane words, 2^20 - 1 surplus ones, the plane turn[1] ending past 2^32 bytes; the world
    at the box's start (k = 0) and at its end, where the world's last slice is the second grid row's (k = 1); inside
    z in [-2, 66) the cut box's bits, 0 everywhere else, the cut box's summary"""
    vx, torch = eng
    a = F.rule_launch(F.PLANES_DIMS, 1, F.read_caps())
    assert a.gy == 2 and a.surplus == (1 << 20) - 1 and a.layout.total > 1 << 32  # reached
    rule, want, first = F.planes_expected(outside, k)
    expect = np.ascontiguousarray(want["bits"][0].T).astype(np.uint32)  # [z, y]: one word a row, bit 0
    ctx = _ctx(vx, vxo, small_world(), 8)
    try:
        words, summary = _guarded_rule(torch, ctx, vx, F.PLANES_ORIGINS[k], F.PLANES_DIMS, rule, a.layout)
        inner = words.view(-1, 2)[first:first + expect.shape[0]].cpu().numpy().view(np.uint32)
        count = int(torch.count_nonzero(words))
        print("planes", k, outside, summary, "nonzero words", count, "unequal inner words", int((inner != expect).sum()))
        assert np.array_equal(inner, expect) and count == int(expect.sum()) > 0
        assert summary == want["summary"]
        del words
    finally:
        ctx.close()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("outside", (0, 1))
@pytest.mark.parametrize("k", (0, 1))
def test_rule_rows_of_millions_of_words(eng, vxo, k, outside):
    """case 2: a row of 2^28 voxels that ends three voxels past the world's far x face, and two rows of 2^27 - 59 that start
    seven voxels before its near one: the four words around the world are the window's, every other word is 0"""
    vx, torch = eng
    o, d = F.ROWS_BOXES[k]
    a = F.rule_launch(d, 1, F.read_caps())
    assert a.layout.wh == ((1 << 23) + 1, (1 << 22) - 1)[k]
    rule, want = F.rows_expected(k, outside)
    first = F.rows_first_word(k)
    expect = pack_region(want["bits"]).reshape(d[1] * d[2], F.ROWS_WINDOW)
    ctx = _ctx(vx, vxo, small_world(), 8)
    try:
        words, summary = _guarded_rule(torch, ctx, vx, o, d, rule, a.layout)
        got = words.view(d[1] * d[2], a.layout.mw)[:, first:first + F.ROWS_WINDOW].cpu().numpy().view(np.uint32)
        count = int(torch.count_nonzero(words))
        print("rows", k, outside, summary, "nonzero words", count, got.tolist())
        assert np.array_equal(got, expect) and count == np.count_nonzero(expect) >= 2
        assert summary == want["summary"]
        del words
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def test_rule_output_launch_in_its_middle_branch(eng, vxo):
    """case 3: 490 000 output words, 239 workgroups, every lane on up to nine words in turn"""
    vx, torch = eng
    a = F.rule_launch(F.REGIME_DIMS, 1, F.read_caps())
    assert (a.few, a.grid, a.regime) == (239, 239, "share")
    ctx = _ctx(vx, vxo, F.regime_world(), F.REGIME_WORLD[3])
    try:
        for k in range(len(F.REGIME_RULES)):
            rule, want = F.regime_expected(k)
            r = ctx.apply_rule(F.REGIME_ORIGIN, F.REGIME_DIMS, _rule(vx, rule))
            got = r.grid()
            print("regime", rule, tuple(r.summary), int((got != want["bits"]).sum()))
            assert np.array_equal(got, want["bits"]) and tuple(r.summary) == want["summary"], rule
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def board(eng, vxo):
    """the 1024 x 1024 x 256 parity checkerboard built on the device, as tests/test_gpu_read_limits.py builds it: (the
    context, the word of every row [z * y, 1])"""
    vx, torch = eng
    dims = F.CHECKER_WORLD[:3]
    ctx = vx.Context(0)
    ctx.build_world(vxo.GEN_INT_TERRAIN, *F.CHECKER_WORLD)
    rows = torch.from_numpy(checker_stamp_rows(dims).view(np.int32).copy()).cuda().reshape(-1, 1)
    bits = rows.expand(-1, dims[0] // 32).contiguous().view(-1)
    st = ctx.edit_stamps([vx.Stamp((0, 0, 0), bits, 0, dims)])
    assert st.bricks_live == dims[0] * dims[1] * dims[2] // 32 ** 3
    del bits
    yield ctx, rows
    ctx.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nb", F.NEIGHBOURHOODS)
def test_rule_counters_at_2_28(eng, board, nb):
    """case 4: every voxel of 2^28 changes at every step: the complement after an odd number of steps, the board after an
    even one; changed_last is 2^28; the output launch is cut to 1024 workgroups"""
    vx, torch = eng
    ctx, rows = board
    dims = F.CHECKER_WORLD[:3]
    assert F.rule_launch(dims, 1, F.read_caps()).few > F.rule_launch(dims, 1, F.read_caps()).grid == 1024
    for i, (scope, n) in enumerate(F.COUNTER_RUNS):
        rule = F.flip_rule(nb, scope, n, (i + nb) & 1)
        r = ctx.apply_rule((0, 0, 0), dims, _rule(vx, rule))
        summary = tuple(r.summary)
        bad = int((r.bits.view(-1, dims[0] // 32) != (~rows if n % 2 else rows)).sum())
        print("checkerboard", rule, summary, "unequal words", bad)
        assert summary == F.checker_summary(dims, n) and bad == 0, rule
        del r
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def sides(eng, vxo):
    """contexts that hold the worlds of three different sides, by brick edge"""
    vx, torch = eng
    held = {}

    def get(factor):
        if factor not in held:
            held[factor] = new_ctx(vx)
            held[factor].SetOrthoWindowSize(*LC.ORTHO_SIZE)
            upload(held[factor], vxo.World.from_voxels(F.sides_world(factor), factor))
        return held[factor]

    yield get
    for c in held.values():
        c.close()


@pytest.mark.parametrize("factor", sorted(F.SIDES_WORLDS))
def test_rule_on_a_world_of_three_different_sides(eng, sides, factor):
    """case 5: boxes over all six faces (brick edge 8), over the y-hi face alone, over the z-hi face alone and over the three
    far faces; BOX with a mask and WORLD; the small boxes through the host form as well"""
    vx, torch = eng
    ctx = sides(factor)
    for k in range(4):
        for s in range(len(F.SIDES_SCOPES)):
            o, d, rule, mask, want = F.sides_expected(factor, k, s)
            r = ctx.apply_rule(o, d, _rule(vx, rule), mask)
            got = r.grid()
            print("sides", factor, o, d, rule, tuple(r.summary), int((got != want["bits"]).sum()))
            assert np.array_equal(got, want["bits"]) and tuple(r.summary) == want["summary"], (factor, k, s)
            if k in (1, 2):
                host = ctx.apply_rule_host(o, d, _rule(vx, rule), mask)
                assert np.array_equal(host.grid(), want["bits"]) and tuple(host.summary) == want["summary"], (factor, k, s)


# ---- frames
def _cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _assert_launches(torch, Wf, Hf):
    """which of `need` and the device's share binds in the counted launch of this device, restated; the tall frame's waves
    walk several tiles on any device of fewer than 2048 compute units"""
    caps, cus = F.read_caps(), _cus(torch)
    counted, plain = F.frame_launch(Wf, Hf, True, cus, caps), F.frame_launch(Wf, Hf, False, cus, caps)
    print("frame launch", (Wf, Hf), "cus", cus, vars(counted), "plain workgroups", plain.grid)
    assert plain.grid == counted.tiles == (2048 if Wf > Hf else 16384) and counted.grid == min(F.ceil_div(counted.tiles, 4), 2 * cus)
    assert counted.binds == ("need" if F.ceil_div(counted.tiles, 4) < 2 * cus else "cus")
    if Hf > Wf:
        assert cus < 2048 and counted.binds == "cus" and counted.per_wave == F.ceil_div(16384, 8 * cus) > 1


@pytest.fixture(scope="module")
def frame_ctx(eng):
    vx, _ = eng
    c = new_ctx(vx)
    c.SetOrthoWindowSize(*T.ORTHO_SIZE)
    yield c
    c.close()


@pytest.mark.parametrize("ortho", (False, True))
@pytest.mark.parametrize("Wf,Hf", F.THIN_FRAMES)
def test_reprojection_of_frames_of_the_longest_side(eng, frame_ctx, Wf, Hf, ortho):
    """case 6: the counted and the plain launch; every record, colour and framebuffer byte and the summary; guard words
    behind every buffer"""
    vx, torch = eng
    _assert_launches(torch, Wf, Hf)
    case, rec, summary = F.thin_reproject(Wf, Hf, ortho)
    for counted in (True, False):
        col, col_all = _guarded(torch, case["color"])
        keys, keys_all = _guarded(torch, case["keys"])
        hist, hist_all = _guarded(torch, case["hist"])
        kprev, kprev_all = _guarded(torch, case["keys_prev"])
        out_hist, out_hist_all = _guarded(torch, case["hist"], PATTERN)
        out, out_all = _guarded(torch, case["color"], PATTERN)
        fb, fb_all = _guarded(torch, case["keys"], PATTERN)
        got = frame_ctx.reproject_frame(col, keys, case["cur"], case["prev"], history=hist, prev_keys=kprev, max_history=case["max_history"],
                                        ortho=ortho, out_history=out_hist, out=out, fb=fb, summary=counted)
        torch.cuda.synchronize()
        what = (Wf, Hf, ortho, counted)
        bad = RD.bits(got.history.cpu().numpy()) != RD.bits(rec)
        print("thin reprojection", what, summary, "unequal", int(bad.sum()), np.argwhere(bad)[:3].tolist())
        assert not bad.any(), what
        assert np.array_equal(RD.bits(got.color.cpu().numpy()), RD.bits(rec[..., :3])), what
        assert np.array_equal(fb.cpu().numpy().view(np.uint8).reshape(Hf, Wf, 4), RD.bgra8(rec[..., :3])), what
        assert (tuple(got.summary) == summary) if counted else got.summary is None, what
        for whole in (col_all, keys_all, hist_all, kprev_all, out_hist_all, out_all, fb_all):
            assert _guards_ok(torch, whole), what


def _light_call(torch, ctx, case, Wf, Hf, counted, alias=False, flags=None, field=None, box=None):
    """vxrt_light_frame through the Python mirror, guard words behind every buffer: (colour, framebuffer, terms, summary);
    `field` and `box`: device levels and their box in place of the case's"""
    col, col_all = _guarded(torch, case["color"])
    keys, keys_all = _guarded(torch, case["keys"])
    hit, hit_all = _guarded(torch, case["hit"].view(np.int32).reshape(Hf, 2 * Wf))
    whole = [col_all, keys_all, hit_all]
    if field is None and case["levels"] is not None:
        lev = np.ascontiguousarray(case["levels"].transpose(2, 1, 0)).reshape(-1)
        levels, levels_all = _guarded(torch, np.concatenate([lev, np.zeros((-lev.size) % 4, np.uint8)]).view(np.int32))
        field = levels.view(torch.uint8)
        whole.append(levels_all)
    out, out_all = _guarded(torch, case["color"], PATTERN)
    fb, fb_all = _guarded(torch, case["keys"], PATTERN)
    terms, terms_all = _guarded(torch, case["color"], PATTERN)
    kw = dict(case["params"]) if flags is None else dict(case["params"], flags=flags)
    got = ctx.light_frame(col, keys, hit.view(torch.int64), case["cam"], field=field, box=box or case["box"], ortho=case["ortho"],
                          out=col if alias else out, fb=fb, terms=terms if counted else False, summary=counted, **kw)
    torch.cuda.synchronize()
    for t in whole + [out_all, fb_all, terms_all]:
        assert _guards_ok(torch, t)
    if not counted:
        assert got.summary is None and bool((terms.view(torch.int32) == PATTERN).all())
    return (got.color.cpu().numpy(), fb.cpu().numpy().view(np.uint8).reshape(Hf, Wf, 4), terms.cpu().numpy() if counted else None,
            tuple(got.summary) if counted else None)


def _assert_light(got, color, terms, summary, what):
    bad = RD.bits(got[0]) != RD.bits(color)
    print("light frame", what, summary, "unequal", int(bad.sum()), np.argwhere(bad)[:3].tolist())
    assert not bad.any(), what
    assert np.array_equal(got[1], RD.bgra8(color)), what
    if got[3] is not None:
        assert np.array_equal(RD.bits(got[2]), RD.bits(terms)) and got[3] == summary, what


@pytest.mark.parametrize("ortho", (False, True))
@pytest.mark.parametrize("Wf,Hf", F.THIN_FRAMES)
def test_light_on_frames_of_the_longest_side(eng, vxo, Wf, Hf, ortho):
    """case 6: the counted launch with terms and the plain launch without; every colour, framebuffer byte and term and the
    summary; guard words behind every buffer"""
    vx, torch = eng
    _assert_launches(torch, Wf, Hf)
    case, color, terms, summary = F.thin_light(Wf, Hf, ortho)
    ctx = new_ctx(vx)
    try:
        ctx.SetOrthoWindowSize(*case["ortho_size"])
        upload(ctx, vxo.World.from_voxels(case["world"], 8))
        for counted in (True, False):
            _assert_light(_light_call(torch, ctx, case, Wf, Hf, counted), color, terms, summary, (Wf, Hf, ortho, counted))
    finally:
        ctx.close()


@pytest.mark.parametrize("factor", sorted(F.SIDES_WORLDS))
def test_light_on_a_world_of_three_different_sides(eng, sides, factor):
    """case 11: hit voxels on all six boundary layers of a world with X > Z > Y, a light box over its y-hi and z-hi faces"""
    vx, torch = eng
    ctx = sides(factor)
    Wf, Hf = F.LIGHT_SIDES_FRAME
    for ortho in (False, True) if factor == 8 else (False,):
        case, color, terms, summary, _ = F.light_sides_case(factor, ortho)
        _assert_light(_light_call(torch, ctx, case, Wf, Hf, True, alias=ortho), color, terms, summary, (factor, ortho))


@pytest.fixture(scope="module")
def small_light_ctx(eng, vxo):
    """the 64^3 world of tests/light_frame_cases.py's random cases"""
    vx, _ = eng
    c = new_ctx(vx)
    c.SetOrthoWindowSize(*LC.ORTHO_SIZE)
    upload(c, vxo.World.from_voxels(LC.random_case(8, 8, False)["world"], 8))
    yield c
    c.close()


@pytest.mark.parametrize("k", range(len(F.LIGHT_BOXES)))
def test_light_boxes_at_their_limits(eng, small_light_ctx, k):
    """case 10: a row of 2^28 bytes that ends next to the world, a slab of kLfMaxBoxVoxels bytes whose last slices hold the
    world, and a box at x = -2^31; every byte that no cell near the world names is poison"""
    vx, torch = eng
    case, color, terms, summary, _ = F.light_box_case(k)
    origin, dims = F.LIGHT_BOXES[k]
    n = dims[0] * dims[1] * dims[2]
    field = torch.full((n + 256,), F.LIGHT_BOX_POISON, dtype=torch.uint8, device="cuda")
    field[n:] = 0x5A
    cut = F.near_box(F.LIGHT_BOXES[k])
    if cut is not None:
        r = np.stack(np.meshgrid(*(np.arange(a, a + m, dtype=np.int64) for a, m in zip(cut[2], cut[1])), indexing="ij"), -1)
        at = r[..., 0] + dims[0] * (r[..., 1] + dims[1] * r[..., 2])
        assert at.min() > (1 << 28) - (1 << 19) and at.max() < n
        field[torch.from_numpy(at.reshape(-1)).cuda()] = torch.from_numpy(case["levels"].reshape(-1).copy()).cuda()
    try:
        got = _light_call(torch, small_light_ctx, case, *F.LIGHT_BOX_FRAME, True, field=field[:n], box=F.LIGHT_BOXES[k])
        _assert_light(got, color, terms, summary, ("light box", k))
        assert (got[3][1] == 0) == (k == 2) and bool((field[n:] == 0x5A).all())
    finally:
        del field
        torch.cuda.empty_cache()


@pytest.mark.parametrize("ortho", (False, True))
def test_reprojection_of_special_operands(eng, frame_ctx, ortho):
    """case 8, against the restatement that tests/test_rule_frame_limits_host.py holds to its scalar twin; counted and plain"""
    vx, torch = eng
    Wf, Hf = F.SPECIAL_FRAME
    dev = lambda a: torch.from_numpy(np.array(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()
    for k in range(len(F.SPECIAL_REPROJECT)):
        case, rec, summary, _ = F.special_reproject(ortho, k)
        for counted in (True, False):
            fb = torch.zeros((Hf, Wf, 4), dtype=torch.uint8, device="cuda")
            got = frame_ctx.reproject_frame(dev(case["color"]), dev(case["keys"]), case["cur"], case["prev"], dev(case["hist"]), dev(case["keys_prev"]),
                                            case["max_history"], ortho=ortho, fb=fb, summary=counted)
            torch.cuda.synchronize()
            what = (ortho, k, counted)
            bad = RD.bits(got.history.cpu().numpy()) != RD.bits(rec)
            print("special reprojection", what, summary, "unequal", int(bad.sum()), np.argwhere(bad)[:3].tolist())
            assert not bad.any(), what
            assert np.array_equal(RD.bits(got.color.cpu().numpy()), RD.bits(rec[..., :3])), what
            assert np.array_equal(fb.cpu().numpy(), RD.bgra8(rec[..., :3])), what
            assert (tuple(got.summary) == summary) if counted else got.summary is None, what


@pytest.mark.parametrize("ortho", (False, True))
def test_light_on_special_operands(eng, vxo, ortho):
    """case 8: both parameter sets, the four flag sets, axis fields 3 and 31, planes 0 and 0x1FFFFFF, the straight-down camera"""
    vx, torch = eng
    world = F.special_light(ortho, 0)[0]["world"]
    ctx = new_ctx(vx)
    try:
        ctx.SetOrthoWindowSize(*LC.ORTHO_SIZE)
        upload(ctx, vxo.World.from_voxels(world, 8))
        for k, (_, flags, _) in enumerate(F.SPECIAL_LIGHT):
            case, color, terms, summary = F.special_light(ortho, k)
            assert np.array_equal(case["world"], world)
            _assert_light(_light_call(torch, ctx, case, *F.SPECIAL_FRAME, True, alias=bool(k & 1), flags=flags), color, terms, summary,
                          ("special light", ortho, k))
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def large_world(eng):
    """a context with the device-built 8192 x 512 x 8192 bench world, and solid(q) for tests/ref_light_frame.py: one
    vxrt_read_region of the whole world (2^30 words) kept on the device and looked up there"""
    vx, torch = eng
    X, Y, Z = F.GUIDE_WORLD[:3]
    c = new_ctx(vx)
    c.SetOrthoWindowSize(*F.LARGE_ORTHO)
    c.build_world(vx.GEN_PERLIN_REF, *F.GUIDE_WORLD)
    words = c.read_region((0, 0, 0), (X, Y, Z))
    torch.cuda.synchronize()
    assert words.numel() == X * Y * Z // 32

    def solid(q):
        t = torch.from_numpy(np.ascontiguousarray(q.reshape(-1, 3), np.int64)).cuda()
        w = words[(t[:, 0] >> 5) + (X // 32) * (t[:, 1] + Y * t[:, 2])]
        return (((w >> (t[:, 0] & 31).to(torch.int32)) & 1) != 0).cpu().numpy().reshape(q.shape[:-1])

    yield c, solid
    c.close()
    del words
    torch.cuda.empty_cache()


@pytest.mark.parametrize("index", range(len(F.GUIDE_FRAMES)))
def test_light_on_the_bench_world(eng, vxo, large_world, index):
    """case 9: hit indices of 2^32 and more, on the world's six boundary layers and in the corner the light box covers; the
    keys are vxrt_frame_guides' (equal to the restatement's); the restatement's solidity comes from vxrt_read_region, which
    has its own tests, and not from lf_solid"""
    vx, torch = eng
    ctx, solid = large_world
    dims = F.GUIDE_WORLD[:3]
    total = dims[0] * dims[1] * dims[2]
    Wf, Hf = F.GUIDE_FRAMES[index]
    for ortho in (False, True):
        cam = helpers.camera("AD"[ortho], dims, vxo)
        hit, kinds = F.large_hits(Wf, Hf, 2 * index + ortho)
        assert ((hit >= 1 << 32) & (hit < total)).sum() > 1000 and (kinds == 6).sum() > 300
        keys = ctx.frame_guides(Wf, Hf, *cam, torch.from_numpy(hit).cuda(), ortho=ortho).cpu().numpy().view(np.uint32).reshape(Hf, Wf)
        o, d = RD.primary_rays(Wf, Hf, *cam, ortho=ortho, ortho_size=F.LARGE_ORTHO)
        assert np.array_equal(keys, RD.keys_np(hit, dims, o, d))
        color, _ = RD.random_frame(Wf, Hf, 3)
        case = dict(color=color, keys=keys, hit=hit, cam=cam, ortho=ortho, levels=F.large_levels(), box=F.LARGE_BOX, params=dict(LC.PARAMS))
        want = LF.light_frame_np(color, keys, hit, o, d, dims, case["levels"], case["box"], case["params"], solid=solid)
        assert want[2][1] > 100 and want[2][2] > 100 and want[2][0] - want[2][2] > 100 and (want[3]["hit"] & want[3]["front_outside_world"]).sum() > 50
        for counted in (True, False):
            _assert_light(_light_call(torch, ctx, case, Wf, Hf, counted), *want[:3], ("bench world", (Wf, Hf), ortho, counted))


def test_reprojection_at_the_pixel_limit(eng, frame_ctx):
    """case 7: 8190 x 8194 pixels, every input a hash of the pixel index evaluated on the device; the counted launch (129
    tiles a wave on 256 compute units) and the plain one bit-equal, the counters consistent over the whole frame, no output
    word left as it was, and five bands of six rows bit-equal to the banded restatement"""
    vx, torch = eng
    Wf, Hf = F.LIMIT_FRAME
    n = Wf * Hf
    shape = F.frame_launch(Wf, Hf, True, _cus(torch), F.read_caps())
    print("pixel limit launch", vars(shape))
    assert shape.tiles == 128 * 2049 and shape.per_wave > 16
    table = lambda v: torch.tensor(v, dtype=torch.float32 if isinstance(v[0], float) else torch.int64, device="cuda")
    signed = lambda k: (k - ((k >> 31) << 32)).to(torch.int32)
    color, keys, rgb, nn, kprev = F.limit_reproject_inputs(torch.arange(n, dtype=torch.int64, device="cuda"), table, lambda x: x.to(torch.float32))
    keys, kprev = signed(keys), signed(kprev)
    hist = torch.cat([rgb, nn[:, None]], 1).contiguous()
    del rgb, nn
    cur, prev = F.limit_cameras()
    outs = []
    try:
        for counted in (True, False):
            oh = torch.full((4 * n + 64,), PATTERN, dtype=torch.int32, device="cuda")
            oc = torch.full((3 * n + 64,), PATTERN, dtype=torch.int32, device="cuda")
            fb = torch.full((n + 64,), PATTERN, dtype=torch.int32, device="cuda")
            got = frame_ctx.reproject_frame(color.view(Hf, Wf, 3), keys, cur, prev, history=hist.view(Hf, Wf, 4), prev_keys=kprev,
                                            max_history=F.LIMIT_MAX_HISTORY, out_history=oh[:4 * n].view(torch.float32).view(Hf, Wf, 4),
                                            out=oc[:3 * n].view(torch.float32).view(Hf, Wf, 3), fb=fb[:n], summary=counted)
            torch.cuda.synchronize()
            for t in (oh, oc, fb):
                assert bool((t[-64:] == PATTERN).all()) and not bool((t[:-64] == PATTERN).any()), counted
            outs.append((oh, oc, fb, tuple(got.summary) if counted else None))
        (oh, oc, fb, summary), plain = outs
        assert torch.equal(oh, plain[0]) and torch.equal(oc, plain[1]) and torch.equal(fb, plain[2])
        print("pixel limit", summary)
        assert summary[0] == int(torch.count_nonzero(keys)) and summary[0] == summary[1] + summary[2] + summary[3] and min(summary) > 1 << 20
        counts = np.zeros(4, np.int64)
        for y0 in F.limit_bands():
            rec, s = F.limit_reproject_band(y0)
            rows = slice(y0 * Wf, (y0 + F.LIMIT_BAND) * Wf)
            got = oh[:4 * n].view(n, 4)[rows].cpu().numpy().view(F32).reshape(rec.shape)
            bad = RD.bits(got) != RD.bits(rec)
            print("pixel limit band", y0, s, "unequal", int(bad.sum()), np.argwhere(bad)[:3].tolist())
            assert not bad.any(), y0
            assert np.array_equal(RD.bits(oc[:3 * n].view(n, 3)[rows].cpu().numpy().view(F32)), RD.bits(rec[..., :3].reshape(-1, 3))), y0
            assert np.array_equal(fb[:n][rows].cpu().numpy().view(np.uint8).reshape(F.LIMIT_BAND, Wf, 4), RD.bgra8(rec[..., :3])), y0
    finally:
        del outs, color, keys, kprev, hist
        torch.cuda.empty_cache()


def test_light_at_the_pixel_limit(eng, small_light_ctx):
    """case 7 for the light on frames: hit indices and colours hashed from the pixel index on the device, the keys from
    vxrt_frame_guides (equal to the restatement's on the bands); counted and plain launch bit-equal, hit the number of
    non-zero keys, the other counters at most hit, no output word left as it was, five bands against the restatement"""
    vx, torch = eng
    Wf, Hf = F.LIMIT_FRAME
    n = Wf * Hf
    case = LC.random_case(8, 8, False)
    table = lambda v: torch.tensor(v, dtype=torch.float32 if isinstance(v[0], float) else torch.int64, device="cuda")
    color, hit = F.limit_light_inputs(torch.arange(n, dtype=torch.int64, device="cuda"), table, lambda x: x.to(torch.float32))
    color, hit = color.contiguous(), hit.contiguous()
    keys = small_light_ctx.frame_guides(Wf, Hf, *case["cam"], hit, ortho=False)
    levels = torch.from_numpy(np.ascontiguousarray(case["levels"].transpose(2, 1, 0))).cuda()
    outs = []
    try:
        for counted in (True, False):
            oc = torch.full((3 * n + 64,), PATTERN, dtype=torch.int32, device="cuda")
            fb = torch.full((n + 64,), PATTERN, dtype=torch.int32, device="cuda")
            tm = torch.full((3 * n + 64,), PATTERN, dtype=torch.int32, device="cuda")
            got = small_light_ctx.light_frame(color.view(Hf, Wf, 3), keys, hit, case["cam"], field=levels, box=case["box"],
                                              out=oc[:3 * n].view(torch.float32).view(Hf, Wf, 3), fb=fb[:n],
                                              terms=tm[:3 * n].view(torch.float32).view(Hf, Wf, 3) if counted else False, summary=counted, **case["params"])
            torch.cuda.synchronize()
            for t in (oc, fb) + ((tm,) if counted else ()):
                assert bool((t[-64:] == PATTERN).all()) and not bool((t[:-64] == PATTERN).any()), counted
            outs.append((oc, fb, tm, tuple(got.summary) if counted else None))
        (oc, fb, tm, summary), plain = outs
        assert torch.equal(oc, plain[0]) and torch.equal(fb, plain[1]) and bool((plain[2] == PATTERN).all())
        print("pixel limit light", summary)
        assert summary[0] == int(torch.count_nonzero(keys)) > 1 << 25 and all(0 < v <= summary[0] for v in summary[1:])
        for y0 in F.limit_bands():
            kb, cb, tb, s = F.limit_light_band(y0)
            rows = slice(y0 * Wf, (y0 + F.LIMIT_BAND) * Wf)
            assert np.array_equal(keys.view(-1)[rows].cpu().numpy().view(np.uint32).reshape(kb.shape), kb), y0
            bad = RD.bits(oc[:3 * n].view(n, 3)[rows].cpu().numpy().view(F32).reshape(cb.shape)) != RD.bits(cb)
            print("pixel limit light band", y0, s, "unequal", int(bad.sum()), np.argwhere(bad)[:3].tolist())
            assert not bad.any(), y0
            assert np.array_equal(RD.bits(tm[:3 * n].view(n, 3)[rows].cpu().numpy().view(F32).reshape(tb.shape)), RD.bits(tb)), y0
            assert np.array_equal(fb[:n][rows].cpu().numpy().view(np.uint8).reshape(F.LIMIT_BAND, Wf, 4), RD.bgra8(cb)), y0
    finally:
        del outs, color, hit, keys
        torch.cuda.empty_cache()
