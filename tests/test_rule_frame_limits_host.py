"""The rule and frame limit cases (tests/rule_frame_limit_cases.py) without a GPU: the launch caps read from the sources,
every case past the cap it targets, a copy of the sources with any one cap raised 64-fold leaving some case short (so raising
a cap fails here instead of quietly emptying tests/test_gpu_rule_frame_limits.py), the rule's launch arithmetic restated and
held to the figures worked out by hand and to rule_layout itself (tests/tools/rule_check.cpp), the identities of the large
cases held against tests/ref_rule.py at small sizes, and the cases that the host harnesses can run in seconds through the
kernels' own code with every index checked: the worlds of three different sides (rule_check, lightframe_check), the
frames of 65535 pixels a side (reproject_check, lightframe_check) with waves that walk hundreds of tiles, and the special
operands, on which the vectorised and the scalar restatements are held to agree as well."""
import os
import re

import numpy as np
import pytest

from tests import ref_denoise as RD
from tests import ref_rule as R
from tests import rule_frame_limit_cases as F
from tests.helpers import build_harness
from tests.read_limit_cases import checker
from tests.test_light_frame_host import _assert_equal as _light_equal
from tests.test_light_frame_host import _run as _light_harness
from tests.test_reproject_host import _assert_equal as _reproject_equal
from tests.test_reproject_host import _run as _reproject_harness
from tests.test_rule_host import _layout, _run_harness


def _short(caps):
    return [(case.name, what, value, bound) for case in F.LAUNCH_CASES for what, value, bound in case.reach(caps)
            if not value > bound]


# ---- the caps --------------------------------------------------------------------------------------------------------------
def test_caps_are_read_from_the_sources():
    c = F.read_caps()
    assert all(v > 0 for v in c.values())
    assert (c["rule_max_iterations"], c["dn_max_side"]) == (R.MAX_ITERATIONS, RD.MAX_SIDE)
    assert c["rp_plain"] // 64 == 4 and c["rp_counted"] % c["rp_plain"] == 0  # the tile of rp_tiles: 64 x 4 pixels, one row a wave
    assert all(RD.frame_ok(*f) for f in F.THIN_FRAMES)


def test_the_launch_restatement_gives_the_figures_worked_out_by_hand():
    c = F.read_caps()
    # case 1: halo 3 x 4 x (2^26 + 2), one word a row: 4 * (2^26 + 2) = 2^28 + 8 words, 2^20 + 1 workgroups
    a = F.rule_launch(F.PLANES_DIMS, 1, c)
    assert (a.layout.hd, a.layout.wh, a.layout.np, a.layout.nb) == ((3, 4, (1 << 26) + 2), 1, (1 << 28) + 8, 1 << 27)
    assert (a.blocks, a.gx, a.gy, a.surplus) == ((1 << 20) + 1, 1 << 20, 2, (1 << 20) - 1)
    plane = (1 << 30) + 256  # 2^30 + 32 bytes, up to the next multiple of 256
    assert (a.layout.free, a.layout.turn, a.layout.total) == (plane, (2 * plane, 3 * plane), 4 * plane)
    assert a.layout.turn[1] < 1 << 32 < a.layout.turn[1] + 4 * a.layout.np and a.layout.total == (1 << 32) + 1024
    assert (a.tb, a.few, a.grid, a.regime, a.strides) == (1 << 19, 1 << 16, 1024, "share", 512)
    # case 2: halo rows of 2^28 + 2 and 2^27 - 57 voxels
    b, e = (F.rule_launch(d, 1, c) for _, d in F.ROWS_BOXES)
    assert (b.layout.wh, b.layout.np, b.layout.mw, b.layout.nb) == ((1 << 23) + 1, 9 * ((1 << 23) + 1), 1 << 23, 1 << 23)
    assert (e.layout.wh, e.layout.np, e.layout.mw, e.layout.nb) == ((1 << 22) - 1, 12 * ((1 << 22) - 1), (1 << 22) - 1, (1 << 23) - 2)
    assert 2 * F.ROWS_BOXES[1][1][0] == (1 << 28) - 118 and F.ROWS_BOXES[1][1][0] % 32 == 5
    assert (b.blocks, b.gy, b.tb, b.few, b.grid) == (294913, 1, 1 << 15, 1 << 12, 1024) and (e.tb, e.few, e.strides) == (1 << 15, 1 << 12, 32)
    o, d = F.ROWS_BOXES[0]
    assert o[0] + d[0] - 1 == 64 + 2 and F.rows_first_word(0) == (1 << 23) - 4 and F.row_window(o, d, F.rows_first_word(0), 4) == ((-61, 10, 20), (128, 1, 1))
    assert F.row_window(*F.ROWS_BOXES[1], 0, 4) == ((-7, 10, 20), (128, 2, 1))
    # case 3: 490 000 output words, 1915 blocks, 239 workgroups of the middle branch, nine words in turn a lane
    g = F.rule_launch(F.REGIME_DIMS, 1, c)
    assert (g.layout.nb, g.tb, g.few, g.grid, g.regime, g.strides) == (490000, 1915, 239, 239, "share", 9)
    assert F.rule_launch(F.REGIME_DIMS, 2, c).grid == 239  # (the output's grid does not depend on the halo)
    s, f = F.rule_launch(F.REGIME_SMALL, 1, c), F.rule_launch(F.REGIME_FLOOR, 1, c)
    assert (s.tb, s.few, s.regime) == (1, 1, "all") and (f.tb, f.few, f.regime) == (352, 128, "floor")
    assert [F.rule_launch((32 * 256 * n, 1, 1), 1, c).few for n in (127, 128, 1023, 1024, 8191, 8192, 8200)] == [127, 128, 128, 128, 1023, 1024, 1025]
    # case 4: 2^23 output words, 2^15 blocks, 4096 workgroups cut to 1024, 32 words in turn a lane; WORLD with 16 iterations
    k = F.rule_launch(F.CHECKER_WORLD[:3], 1, c)
    assert (k.layout.nb, k.tb, k.few, k.grid, k.strides) == (1 << 23, 1 << 15, 4096, 1024, 32)
    assert F.rule_layout(F.CHECKER_WORLD[:3], 16).hd == (1056, 1056, 288) and F.rule_launch(F.CHECKER_WORLD[:3], 16, c).gy == 1
    assert F.checker_summary(F.CHECKER_WORLD[:3], 3)[:5] == (1 << 27,) * 4 + (1 << 28,)
    # case 6: 1024 x 2 and 1 x 16384 tiles; 512 workgroups of four tile groups on 256 compute units
    w, t = (F.frame_launch(*fr, True, 256, c) for fr in F.THIN_FRAMES)
    assert (w.across, w.down, w.tiles, w.grid, w.per_wave) == (1024, 2, 2048, 512, 1) and (t.across, t.down, t.tiles, t.grid, t.per_wave, t.binds) == (1, 16384, 16384, 512, 8, "cus")
    assert F.frame_launch(*F.THIN_FRAMES[0], True, 304, c).binds == "need" and F.frame_launch(*F.THIN_FRAMES[0], False, 256, c).grid == 2048
    assert [F.frame_launch(*fr, True, F.THIN_HOST_CUS, c).per_wave for fr in F.THIN_FRAMES] == [86, 683]


@pytest.fixture(scope="module")
def rule_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "rule_check")


def test_the_layout_restatement_is_rule_layout(rule_harness, tmp_path):
    """the byte count of vxrt_rule.hpp's rule_layout (through the harness, which builds no world for it) for the boxes of
    cases 1 to 4"""
    for o, d, n, scope in [(F.PLANES_ORIGIN, F.PLANES_DIMS, 2, R.BOX), (*F.ROWS_BOXES[0], 1, R.BOX), (*F.ROWS_BOXES[1], 1, R.BOX),
                           (F.REGIME_ORIGIN, F.REGIME_DIMS, 2, R.WORLD), ((0, 0, 0), F.CHECKER_WORLD[:3], 16, R.WORLD)]:
        h = n if scope == R.WORLD else 1
        assert _layout(rule_harness, tmp_path, o, d, R.RefRule(R.N26, 2, 2, n, scope, 0)) == (0, True, True, F.rule_layout(d, h).total), (o, d)


@pytest.mark.parametrize("case", F.LAUNCH_CASES, ids=[c.name for c in F.LAUNCH_CASES])
def test_case_exceeds_the_cap_it_targets(case):
    reach = case.reach(F.read_caps())
    assert reach
    for what, value, bound in reach:
        assert value > bound, (case.name, what, value, bound)


@pytest.mark.parametrize("name", F.CAPS_THAT_BIND)
def test_a_raised_cap_leaves_a_case_short(tmp_path, name):
    """each cap multiplied by 64 (a shift count: 64-fold) in a copy of its source: some case no longer exceeds it"""
    for path, _, _ in F.CAP_SOURCES.values():
        dst = tmp_path / path
        dst.parent.mkdir(parents=True, exist_ok=True)
        with open(os.path.join(F.ROOT, path)) as f:
            dst.write_text(f.read())
    path, rx, _ = F.CAP_SOURCES[name]
    text = (tmp_path / path).read_text()
    m = re.search(rx, text)
    raised = re.sub(r"(?<!\d)%s(?!\d)" % m.group(1), str(int(m.group(1)) * 64), m.group(0))  # the number, not its digits in others
    (tmp_path / path).write_text(text.replace(m.group(0), raised))
    caps = F.read_caps(str(tmp_path))
    assert caps[name] >= 64 * F.read_caps()[name]
    assert {k for k in caps if caps[k] != F.read_caps()[k]} == {name}
    assert _short(caps), name
    assert not _short(F.read_caps())


# ---- the identities of the rule cases ----------------------------------------------------------------------------------------
def _same(a, b, what):
    assert np.array_equal(a["bits"], b["bits"]) and a["summary"] == b["summary"], what


def test_a_box_far_longer_than_the_world_along_z_is_its_cut():
    """clipped_z at small sizes: both scopes, both `outside` values, every neighbourhood, the box starting before and
    ending after the world, 1 to 3 iterations"""
    rng = np.random.default_rng(1)
    world = rng.random((20, 18, 12)) < 0.45
    for nb in F.NEIGHBOURHOODS:
        for scope in (R.BOX, R.WORLD):
            for outside in (0, 1):
                for n, (o, d) in zip((1, 2, 3), (((7, 3, -30), (1, 2, 90)), ((-2, 15, -9), (5, 6, 40)), ((11, 5, 2), (3, 4, 50)))):
                    rule = F.lively(rng, world, (5, 5, 2), (9, 9, 9), nb, scope, n, outside)
                    whole = R.apply_rule(world, o, d, rule)
                    co, cd, first = F.clipped_z(o, d, world.shape[2], n)
                    cut = R.apply_rule(world, co, cd, rule)
                    assert first == max(-n - o[2], 0) and cd[2] < d[2]
                    inner = whole["bits"][:, :, first:first + cd[2]]
                    assert np.array_equal(inner, cut["bits"]) and inner.any() and whole["summary"] == cut["summary"], (nb, scope, outside, n)
                    assert not whole["bits"][:, :, :first].any() and not whole["bits"][:, :, first + cd[2]:].any()
    for outside in (0, 1):  # the case's own cuts: 68 slices from z = -2 on, slice 98 of the box; the last 66 slices of the box
        for k, (first, slices) in enumerate(((98, 68), ((1 << 26) - 66, 66))):
            rule, want, at = F.planes_expected(outside, k)
            assert at == first and want["bits"].shape == (1, 2, slices) and want["summary"][2] > 0 and want["summary"][3] > 0
            assert rule.scope == R.BOX and rule.neighbours == R.N26 and rule.iterations == 2 and rule.outside == outside
            assert want["bits"][:, :, -1].any() or k == 0
    # the second origin: the box's last slice is halo slice 2^26, whose four words are words 2^28 .. 2^28 + 3 of a plane
    assert F.PLANES_ORIGINS[1][2] + F.PLANES_DIMS[2] == 64 and 4 * (1 << 26) == 256 * F.read_caps()["grid_2d_x"]


def test_a_box_far_longer_than_the_world_along_x_is_its_window():
    """row_window at small sizes: rows of 40 words that end just past the world's far face and rows that start just before
    its near one, against the restatement on the whole box"""
    rng = np.random.default_rng(2)
    world = rng.random((64, 16, 16)) < 0.4
    for nb in F.NEIGHBOURHOODS:
        for outside in (0, 1):
            for (o, d), first in ((((64 + 3 - 1280, 5, 9), (1280, 1, 1)), 36), (((-7, 5, 9), (1280 + 5, 2, 1)), 0), (((-40, 14, -1), (1000, 3, 3)), 1)):
                rule = F.lively(rng, world, (10, 3, 3), (40, 9, 9), nb, R.BOX, 1, outside)
                whole = R.apply_rule(world, o, d, rule)
                wo, wd = F.row_window(o, d, first, F.ROWS_WINDOW)
                assert wo[0] <= 0 and wo[0] + wd[0] >= 64
                part = R.apply_rule(world, wo, wd, rule)
                x0 = 32 * first
                assert np.array_equal(whole["bits"][x0:x0 + wd[0]], part["bits"]) and part["bits"].any() and whole["summary"] == part["summary"]
                assert not whole["bits"][:x0].any() and not whole["bits"][x0 + wd[0]:].any()
    for k in (0, 1):
        for outside in (0, 1):
            rule, want = F.rows_expected(k, outside)
            assert want["summary"][2] > 0 and want["summary"][3] > 0 and (rule.neighbours, rule.iterations, rule.outside) == (R.N18, 1, outside)


def test_the_flip_rule_complements_the_checkerboard_at_every_step():
    dims = (16, 12, 8)
    board = checker(dims)
    for nb in F.NEIGHBOURHOODS:
        for scope, n in F.COUNTER_RUNS + ((R.WORLD, 1), (R.BOX, 3)):
            for outside in (0, 1):
                got = R.apply_rule(board, (0, 0, 0), dims, F.flip_rule(nb, scope, n, outside))
                assert np.array_equal(got["bits"], ~board if n % 2 else board), (nb, scope, n, outside)
                assert got["summary"] == F.checker_summary(dims, n), (nb, scope, n, outside)
    assert F.checker_summary((1024, 1024, 256), 1) == (1 << 27, 1 << 27, 1 << 27, 1 << 27, 1 << 28, (0, 0, 0), (1023, 1023, 255))
    assert F.checker_summary((1024, 1024, 256), 16) == (1 << 27, 1 << 27, 0, 0, 1 << 28, *F.NONE)


def test_the_output_regime_cases_are_lively():
    for k in range(len(F.REGIME_RULES)):
        rule, want = F.regime_expected(k)
        assert want["summary"][2] > 1000 and want["summary"][3] > 1000 and (rule.neighbours, rule.scope, rule.iterations, rule.outside) == F.REGIME_RULES[k]


# ---- worlds of three different sides -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", sorted(F.SIDES_WORLDS))
def test_the_rule_code_on_the_host_on_a_world_of_three_different_sides(rule_harness, tmp_path, factor):
    """every box and scope of case 5 at brick edge 8, the boxes over the y-hi and the z-hi face alone at the larger edges:
    lively by the restatement, the harness equal to it"""
    world = F.sides_world(factor)
    assert len(set(world.shape)) == 3
    seen = set()
    for k in range(4) if factor == 8 else (1, 2):
        for s in range(len(F.SIDES_SCOPES)):
            o, d, rule, mask, want = F.sides_expected(factor, k, s)
            assert want["summary"][2] > 0 and want["summary"][3] > 0 and (mask is None) == (rule.scope == R.WORLD)
            seen.add((rule.neighbours, rule.scope, rule.outside))
            got = _run_harness(rule_harness, tmp_path, world, factor, o, d, rule, mask)
            assert np.array_equal(got["bits"], want["bits"]) and got["summary"] == want["summary"], (factor, k, s)
    if factor == 8:
        assert {nb for nb, _, _ in seen} == set(F.NEIGHBOURHOODS) and {(sc, out) for _, sc, out in seen} == {(a, b) for a in (0, 1) for b in (0, 1)}
        assert F.sides_overhang(8, 0) == (5,) * 6 and F.sides_overhang(8, 1) == (0, 0, 0, 16, 0, 0) and F.sides_overhang(8, 2) == (0, 0, 0, 0, 0, 22)
        assert F.sides_overhang(8, 3) == (0, 34, 0, 5, 0, 12)


@pytest.fixture(scope="module")
def light_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "lightframe_check")


@pytest.mark.parametrize("factor", sorted(F.SIDES_WORLDS))
def test_the_light_frame_code_on_the_host_on_a_world_of_three_different_sides(light_harness, tmp_path, factor):
    """case 11: what the frame exercises (on the restatement alone), the scalar restatement at brick edge 8, the harness"""
    from tests import light_frame_cases as LC
    for ortho in (False, True) if factor == 8 else (False,):
        case, color, terms, summary, info = F.light_sides_case(factor, ortho)
        hit = info["hit"]
        X, Y, Z = case["world"].shape
        v = np.stack([case["hit"] % X, case["hit"] // X % Y, case["hit"] // (X * Y)], -1)
        for side in range(6):  # hit voxels on every boundary layer of the world
            at = hit & (case["edge_side"] == side)
            assert at.sum() > 50 and (v[at][:, side >> 1] == ((X, Y, Z)[side >> 1] - 1 if side & 1 else 0)).all(), side
        assert (hit & (v[..., 2] >= Y)).sum() > 1000 and (hit & (v[..., 1] < Y) & (v[..., 2] >= Y) & case["world"][tuple(np.where(hit[..., None], v, 0).transpose(2, 0, 1))]).sum() > 100
        assert summary[0] > 8000 and summary[1] > 500 and summary[2] > 500 and summary[0] - summary[1] > 500
        assert (hit & info["front_outside_world"]).sum() > 100 and (hit & (info["cells_in_box"] > 0) & (info["cells_in_box"] < 9)).sum() > 10
        if factor == 8:
            b = LC.run_case(case, scalar=True)
            assert np.array_equal(RD.bits(b[0]), RD.bits(color)) and np.array_equal(RD.bits(b[1]), RD.bits(terms)) and b[2] == summary
        _light_equal(_light_harness(light_harness, tmp_path, case, factor=factor), (color, terms, summary), (factor, ortho))


# ---- frames of 65535 pixels a side ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reproject_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "reproject_check")


@pytest.mark.parametrize("Wf,Hf", F.THIN_FRAMES)
def test_the_frame_code_on_the_host_on_thin_frames(reproject_harness, light_harness, tmp_path, Wf, Hf):
    """the counted launch of three compute units (every wave on 86 and 683 tiles) and the plain one, the ortho camera in the
    counted launch and the perspective one in the plain"""
    case, rec, summary = F.thin_reproject(Wf, Hf, True)
    assert min(summary) > 1000
    _reproject_equal(_reproject_harness(reproject_harness, tmp_path, case, cus=F.THIN_HOST_CUS), (rec, summary), (Wf, Hf, "counted"))
    case, rec, summary = F.thin_reproject(Wf, Hf, False)
    assert min(summary) > 1000
    _reproject_equal(_reproject_harness(reproject_harness, tmp_path, case, summary=False), (rec, summary), (Wf, Hf, "plain"))
    case, color, terms, summary = F.thin_light(Wf, Hf, True)
    assert min(summary) > 1000
    _light_equal(_light_harness(light_harness, tmp_path, case, cus=F.THIN_HOST_CUS), (color, terms, summary), (Wf, Hf, "counted"))
    case, color, terms, summary = F.thin_light(Wf, Hf, False)
    assert min(summary) > 1000
    _light_equal(_light_harness(light_harness, tmp_path, case, summary=False), (color, terms, summary), (Wf, Hf, "plain"))


# ---- special operands ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ortho", (False, True))
def test_the_restatements_and_the_host_code_agree_on_special_reprojection_operands(reproject_harness, tmp_path, ortho):
    """case 8: NaN, infinite, negative-zero and denormal colours and history colours, n from NaN to 1e30, max_history 1, 2 and
    65535, keys on plane 0 and on plane 0x1FFFFFF, a previous camera at a pixel's own surface point and one 1e7 voxels away,
    an ortho camera whose rays have two components exactly 0: the vectorised and the scalar restatement bit for bit, and
    the kernel's code on the host against them"""
    from tests import ref_reproject as T
    for k in range(len(F.SPECIAL_REPROJECT)):
        case, rec, summary, _ = F.special_reproject(ortho, k)
        b = T.run_case(case, scalar=True)
        assert np.array_equal(RD.bits(b[0]), RD.bits(rec)) and b[1] == summary and summary[0] == sum(summary[1:]), (ortho, k)
        _reproject_equal(_reproject_harness(reproject_harness, tmp_path, case), (rec, summary), (ortho, k))
    down = F.special_reproject(True, 4)
    o, d = RD.primary_rays(*F.SPECIAL_FRAME, *down[0]["cur"], ortho=True, ortho_size=down[0]["ortho_size"])
    assert (d[..., 0] == 0).all() and (d[..., 2] == 0).all() and down[2][2] > 3000  # the keys of axes 0 and 2 are offscreen
    case = F.special_reproject(ortho, 1)[0]
    assert case["max_history"] == 2 and np.isnan(case["hist"][..., :3]).sum() > 100


@pytest.mark.parametrize("ortho", (False, True))
def test_the_restatements_and_the_host_code_agree_on_special_light_operands(light_harness, tmp_path, ortho):
    """case 8: the same colours, sky_floor 0 and 1, block_color 0 and 3e38, ao_curve of zeros and up to 3e38, outside_level 0
    and 0xFF, the four flag sets, axis fields 3 and 31 (read as 2), planes 0 and 0x1FFFFFF, and the straight-down camera"""
    from tests import light_frame_cases as LC
    results = []
    for k, (p, flags, pose) in enumerate(F.SPECIAL_LIGHT):
        case, color, terms, summary = F.special_light(ortho, k)
        if k in (0, 1, 4, 5):  # (the scalar restatement takes seconds a frame: both parameter sets, flags 3 and 0, both poses)
            b = LC.run_case(case, flags, scalar=True)
            assert np.array_equal(RD.bits(b[0]), RD.bits(color)) and np.array_equal(RD.bits(b[1]), RD.bits(terms)) and b[2] == summary, (ortho, k)
        _light_equal(_light_harness(light_harness, tmp_path, case, flags), (color, terms, summary), (ortho, k))
        results.append(RD.bits(color))
    assert all(not np.array_equal(results[1], r) for r in results[2:5])  # every flag changes something
    assert np.isinf(F.special_light(ortho, 1)[1]).any()  # 3e38 overflows somewhere


# ---- the light box at its limits ----------------------------------------------------------------------------------------------
def test_a_light_box_cut_to_the_cells_near_the_world_lights_the_frame_alike():
    """near_box at sizes the restatement can hold whole: a row, a slab and a box far from the world, every byte outside the
    cut poisoned"""
    from tests import light_frame_cases as LC
    world = LC.random_case(8, 8, False)["world"]
    for k, box in enumerate((((70 - 3000, 30, 30), (3000, 1, 1)), ((0, 0, 64 - 300), (64, 64, 300)), ((-5000, 0, 0), (3000, 1, 1)),
                             ((-9, 60, -40), (20, 30, 50)))):
        case = F.aimed_case(67, 35, world, box, bool(k & 1), 5 + k)
        cut = F.near_box(box)
        whole = np.full(box[1], F.LIGHT_BOX_POISON, np.uint8)
        if cut is None:
            assert case["levels"] is None
        else:
            assert case["box"] == cut[:2]
            whole[tuple(slice(a, a + n) for a, n in zip(cut[2], cut[1]))] = case["levels"]
        a = LC.run_case(case, levels=cut is not None)
        b = LC.run_case(dict(case, levels=whole, box=box))
        assert np.array_equal(RD.bits(a[0]), RD.bits(b[0])) and np.array_equal(RD.bits(a[1]), RD.bits(b[1])) and a[2] == b[2], box
        assert (a[2][1] > 50) == (cut is not None) and a[2][0] > 1500
    for k in range(len(F.LIGHT_BOXES)):
        case, color, terms, summary, info = F.light_box_case(k)
        assert summary[0] > 10000 and (summary[1] > 500) == (k < 2) and (k == 2) == (case["levels"] is None)
        if k < 2:
            assert (info["hit"] & (info["cells_in_box"] > 0) & (info["cells_in_box"] < 9)).sum() > 500 and (info["hit"] & ~info["front_in_box"]).sum() > 100
    assert F.near_box(F.LIGHT_BOXES[0]) == ((-2, 30, 30), (68, 1, 1), ((1 << 28) - 72, 0, 0))
    assert F.near_box(F.LIGHT_BOXES[1]) == ((0, 0, -2), (64, 64, 66), (0, 0, 65536 - 66)) and F.near_box(F.LIGHT_BOXES[2]) is None


# ---- the restatement's additions ------------------------------------------------------------------------------------------------
def test_the_light_restatement_with_a_lookup_in_place_of_the_world():
    """ref_light_frame.light_frame_np with solid=callable(q) and the world's extents gives what it gives with the dense world;
    the hits of case 9 decode to the voxels they were made from"""
    from tests import light_frame_cases as LC
    from tests import ref_light_frame as LF
    for ortho in (False, True):
        case = LC.random_case(67, 35, ortho)
        world = case["world"]
        calls = []

        def lookup(q):
            assert q.shape[-1] == 3 and (q >= 0).all() and (q < world.shape).all()
            calls.append(q.shape)
            return world[q[..., 0], q[..., 1], q[..., 2]]

        a = LC.run_case(case)
        b = LF.light_frame(case["color"], case["hit"], case["cam"], world.shape, case["levels"], case["box"], case["params"], ortho,
                           ortho_size=case["ortho_size"], keys=case["keys"], solid=lookup)
        assert np.array_equal(RD.bits(a[0]), RD.bits(b[0])) and np.array_equal(RD.bits(a[1]), RD.bits(b[1])) and a[2] == b[2] and len(calls) == 9
    hit, kinds = F.large_hits(*F.GUIDE_FRAMES[0])
    X, Y, Z = F.GUIDE_WORLD[:3]
    v = np.stack([hit % X, hit // X % Y, hit // (X * Y)], -1)
    for side in range(6):
        assert (kinds == side).sum() > 100 and (v[kinds == side][:, side >> 1] == ((X, Y, Z)[side >> 1] - 1 if side & 1 else 0)).all()
    assert (kinds == 6).sum() > 300 and (v[kinds == 6] < np.array(F.LARGE_BOX[1]) - 5).all()
    assert set(F.GUIDE_HITS) <= set(hit.reshape(-1)[:len(F.GUIDE_HITS)].tolist())


# ---- the pixel limit -------------------------------------------------------------------------------------------------------------
def test_banded_evaluation_is_a_slice_of_the_whole_frame():
    """case 7: primary_rays and reproject_np with rows=(y0, y1) against the matching rows of the full evaluation on the
    (130, 70) cases; the hashed inputs evaluated by numpy and by torch agree; the bands lie where the case says"""
    import torch
    from tests import ref_reproject as T
    W, H = 130, 70
    for ortho in (False, True):
        case = T.random_case(W, H, ortho)
        full, _ = T.run_case(case)
        o, d = RD.primary_rays(W, H, *case["cur"], ortho=ortho, ortho_size=case["ortho_size"])
        counts = np.zeros(4, np.int64)
        for y0, y1 in ((0, 6), (6, 31), (31, 40), (40, 64), (64, 70)):
            ob, db = RD.primary_rays(W, H, *case["cur"], ortho=ortho, ortho_size=case["ortho_size"], rows=(y0, y1))
            assert np.array_equal(RD.bits(ob), RD.bits(o[y0:y1])) and np.array_equal(RD.bits(db), RD.bits(d[y0:y1]))
            rec, s = T.reproject_np(case["color"][y0:y1], case["keys"][y0:y1], ob, db, case["prev"], T.camera_constants(W, H, 90.0, case["ortho_size"]),
                                    case["hist"], case["keys_prev"], case["max_history"], ortho, rows=(y0, y1), frame_h=H, hist_rows=(0, H))
            assert np.array_equal(RD.bits(rec), RD.bits(full[y0:y1])), (ortho, y0)
            counts += s
        assert tuple(counts) == T.run_case(case)[1]
        with pytest.raises(AssertionError, match="a tap outside the history rows"):  # the history rows given must hold every tap
            T.reproject_np(case["color"][31:40], case["keys"][31:40], o[31:40], d[31:40], case["prev"], T.camera_constants(W, H, 90.0, case["ortho_size"]),
                           case["hist"][34:36], case["keys_prev"][34:36], case["max_history"], ortho, rows=(31, 40), frame_h=H, hist_rows=(34, 36))
    i = np.concatenate([np.arange(0, 3000), np.arange((1 << 25) - 1500, (1 << 25) + 1500), np.arange((1 << 26) - 3004, (1 << 26) - 4)]).astype(np.int64)
    a = F.limit_reproject_inputs(i, lambda v: np.asarray(v, np.float32 if isinstance(v[0], float) else np.int64), lambda x: x.astype(np.float32))
    b = F.limit_reproject_inputs(torch.from_numpy(i), lambda v: torch.tensor(v, dtype=torch.float32 if isinstance(v[0], float) else torch.int64),
                                 lambda x: x.to(torch.float32))
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), y.numpy())
    assert len(np.unique(a[1])) == 5 and (a[4] == F.LIMIT_FOREIGN).sum() > 500 and set(np.unique(a[3]).tolist()) == set(F.LIMIT_N)
    Wf, Hf = F.LIMIT_FRAME
    bands = F.limit_bands()
    assert bands[:3] == (0, Hf - F.LIMIT_BAND, 4095) and bands[2] * Wf < 1 << 25 < (bands[2] + F.LIMIT_BAND) * Wf and Wf * Hf == (1 << 26) - 4
    rec, s = F.limit_reproject_band(bands[2])
    assert rec.shape == (F.LIMIT_BAND, Wf, 4) and min(s) > 1000 and s[0] == s[1] + s[2] + s[3]


def test_the_hashed_light_inputs_of_the_pixel_limit():
    """case 7 for the light on frames: numpy and torch evaluate the same hit indices and colours; every kind occurs; a band of
    the per-pixel restatement is the matching rows of a whole frame (130 x 70: rays of rows=(y0, y1))"""
    import torch
    from tests import light_frame_cases as LC
    i = np.concatenate([np.arange(0, 4000), np.arange((1 << 26) - 4004, (1 << 26) - 4)]).astype(np.int64)
    a = F.limit_light_inputs(i, lambda v: np.asarray(v, np.float32 if isinstance(v[0], float) else np.int64), lambda x: x.astype(np.float32))
    b = F.limit_light_inputs(torch.from_numpy(i), lambda v: torch.tensor(v, dtype=torch.float32 if isinstance(v[0], float) else torch.int64),
                             lambda x: x.to(torch.float32))
    assert np.array_equal(a[0], b[0].numpy()) and np.array_equal(a[1], b[1].numpy()) and a[1].dtype == np.int64
    hit = a[1]
    inside = (hit >= 0) & (hit < 64 ** 3)
    v = np.stack([hit % 64, hit // 64 % 64, hit // 4096], -1)[inside]
    assert (hit == -1).sum() > 500 and (hit >= 64 ** 3).sum() > 500 and (hit >= 1 << 40).sum() > 300 and inside.sum() > 5000
    assert all((v[:, k] == e).sum() > 150 for k in range(3) for e in (0, 63))
    case = LC.random_case(130, 70, False)
    full = LC.run_case(case)
    o, d = RD.primary_rays(130, 70, *case["cam"], rows=(31, 40))
    from tests import ref_light_frame as LF
    part = LF.light_frame_np(case["color"][31:40], case["keys"][31:40], case["hit"][31:40], o, d, case["world"], case["levels"], case["box"], case["params"])
    assert np.array_equal(RD.bits(part[0]), RD.bits(full[0][31:40])) and np.array_equal(RD.bits(part[1]), RD.bits(full[1][31:40]))
    keys, color, terms, s = F.limit_light_band(F.limit_bands()[1])
    assert color.shape == (F.LIMIT_BAND, F.LIMIT_FRAME[0], 3) and s[0] == int((keys != 0).sum()) > 20000 and min(s) > 500
