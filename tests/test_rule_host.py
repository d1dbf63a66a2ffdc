"""CPU checks of the neighbour-count voxel rules (include/vxrt.h, vxrt_apply_rule): the restatements of tests/ref_rule.py
against each other, against brute force and on the hand-derived cases of tests/rule_cases.py, on worlds in which every table
entry decides some voxel, and the kernels' rule code (csrc/vxrt_rule.hpp) compiled for the host (tests/tools/rule_check.cpp)
against them -- bits and summary bit-equal, every index checked -- with the workspace formula and the limits of the
arguments (tests/tools/rule_args_check.cpp)."""
import ctypes as C

import numpy as np
import pytest

from tests import ref_rule as R
from tests import rule_cases as RC
from tests.helpers import build_harness, run_harness, run_harness_files

NEIGHBOURHOODS = (R.N6, R.N18, R.N26)


def _same(a, b, what):
    assert np.array_equal(a["bits"], b["bits"]) and a["summary"] == b["summary"], what


def _both(world, origin, dims, rule, mask=None):
    """the shifted sums and the convolution, asserted equal; returns the first"""
    a = R.apply_rule(world, origin, dims, rule, mask)
    _same(a, R.apply_rule_conv(world, origin, dims, rule, mask), (origin, dims, rule))
    s = a["summary"]
    assert s[1] == s[0] + s[2] - s[3]
    return a


# ---- the restatements --------------------------------------------------------------------------------------------------------
def test_the_neighbourhoods_have_6_18_and_26_offsets():
    for nb in NEIGHBOURHOODS:
        offs = R.offsets(nb)
        assert len(offs) == len(set(offs)) == R.COUNT[nb] and (0, 0, 0) not in offs
        assert int(R._kernel(nb).sum()) == R.COUNT[nb] and R._kernel(nb)[1, 1, 1] == 0


@pytest.mark.parametrize("nb", NEIGHBOURHOODS)
def test_the_restatements_agree_on_random_grids(nb):
    """both scopes, both `outside` values, masks, boxes partly and wholly outside the world"""
    rng = np.random.default_rng(nb)
    w = rng.random((40, 36, 33)) < 0.45
    boxes = [((3, 20, 2), (20, 17, 19)), ((-6, -4, 20), (30, 9, 15)), ((35, 30, 30), (9, 9, 9)), ((-20, 3, 3), (10, 5, 5)),
             ((60, 60, 60), (4, 5, 6)), ((-3, -3, -3), (46, 42, 39))]
    for i, (o, d) in enumerate(boxes):
        for scope in (R.BOX, R.WORLD):
            for outside in (0, 1):
                rule = R.random_rule(rng, nb, 1 + (i + scope + outside) % 3, scope, outside)
                _both(w, o, d, rule)
                if scope == R.BOX:
                    _both(w, o, d, rule, rng.random(d) < 0.5)


def test_the_restatements_equal_brute_force():
    rng = np.random.default_rng(4)
    w = rng.random((9, 8, 10)) < 0.5
    for nb in NEIGHBOURHOODS:
        for o, d in [((2, 2, 3), (4, 3, 4)), ((-2, 5, -1), (5, 5, 4)), ((7, -1, 8), (4, 4, 4)), ((12, 0, 0), (2, 3, 2))]:
            for scope, n in ((R.BOX, 1), (R.BOX, 3), (R.WORLD, 1), (R.WORLD, 2)):
                for outside in (0, 1):
                    rule = R.random_rule(rng, nb, n, scope, outside)
                    mask = rng.random(d) < 0.6 if scope == R.BOX and outside else None
                    _same(_both(w, o, d, rule, mask), R.apply_rule_brute(w, o, d, rule, mask), (o, d, rule))


def test_hand_derived_cases_on_the_restatements():
    for case in RC.all_cases():
        args = (case["world"], case["origin"], case["dims"], case["rule"], case["mask"])
        RC.check(case, _both(*args))
        if case["name"] != "identity":  # (a box of 7200 voxels, three steps: too slow one voxel at a time)
            RC.check(case, R.apply_rule_brute(*args))


def _stamp(world, origin, bits):
    """a REPLACE stamp of `bits` at `origin` on a copy of the world"""
    out = world.copy()
    lo = [max(o, 0) for o in origin]
    hi = [min(o + d, s) for o, d, s in zip(origin, bits.shape, world.shape)]
    if all(a < b for a, b in zip(lo, hi)):
        out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = bits[lo[0] - origin[0]:hi[0] - origin[0], lo[1] - origin[1]:hi[1] - origin[1],
                                                          lo[2] - origin[2]:hi[2] - origin[2]]
    return out


def test_box_scope_of_n_iterations_is_n_calls_with_stamps():
    rng = np.random.default_rng(8)
    w = rng.random((30, 30, 30)) < 0.5
    for nb in NEIGHBOURHOODS:
        for o, d, outside in [((5, 6, 7), (12, 9, 10), 0), ((-3, 20, 25), (10, 14, 9), 1)]:
            rule = R.random_rule(rng, nb, 4, R.BOX, outside)
            mask = rng.random(d) < 0.7
            want = R.apply_rule(w, o, d, rule, mask)
            cur, first = w, None
            for _ in range(4):
                step = R.apply_rule(cur, o, d, rule._replace(iterations=1), mask)
                first = first or step
                cur = _stamp(cur, o, step["bits"])
            assert np.array_equal(want["bits"], step["bits"])
            assert want["summary"][0] == first["summary"][0] and want["summary"][1] == step["summary"][1]
            assert want["summary"][4] == step["summary"][4] and want["summary"][2] > 0 and want["summary"][3] > 0


def test_world_scope_tiles_meet_without_seams():
    """two WORLD windows computed from the same W_0 are the two halves of the window that holds both"""
    rng = np.random.default_rng(12)
    w = rng.random((32, 24, 24)) < 0.5
    rule = R.random_rule(rng, R.N26, 3, R.WORLD)
    whole = R.apply_rule(w, (0, 0, 0), (32, 24, 24), rule)["bits"]
    left, right = R.apply_rule(w, (0, 0, 0), (13, 24, 24), rule)["bits"], R.apply_rule(w, (13, 0, 0), (19, 24, 24), rule)["bits"]
    assert np.array_equal(np.concatenate([left, right]), whole)


# ---- coverage: every table entry decides some voxel ------------------------------------------------------------------------
def test_gradient_worlds_use_every_table_entry():
    seen = {nb: set() for nb in NEIGHBOURHOODS}
    for w, o, d, rule, mask in RC.gradient_cases():
        r = _both(w, o, d, rule, mask)
        assert r["summary"][2] > 0 and r["summary"][3] > 0, rule  # born and died
        seen[rule.neighbours] |= R.pairs_seen(w, o, d, rule, mask)
        if rule.iterations == 1 and mask is None:  # one case per neighbourhood alone shows every pair
            assert R.pairs_seen(w, o, d, rule) == {(s, c) for s in (0, 1) for c in range(R.COUNT[rule.neighbours] + 1)}
    for nb in NEIGHBOURHOODS:
        assert seen[nb] == {(s, c) for s in (0, 1) for c in range(R.COUNT[nb] + 1)}, nb


# ---- the kernels' rule code on the host -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "rule_check")


def _run_harness(harness, tmp_path, world, factor, origin, dims, rule, mask=None):
    from oracle import vxo
    X, Y, Z = world.shape
    header = [0, factor, X, Y, Z, *origin, *dims, rule.neighbours, rule.born, rule.survive, rule.iterations, rule.scope, rule.outside,
              0 if mask is None else 1]
    arrays = [vxo.dense_from_voxels(world)] + ([] if mask is None else [RC.pack(np.asarray(mask, bool))])
    raw, _ = run_harness_files(harness, tmp_path, np.asarray(header, np.int64).astype(np.uint32).view(np.int32), *arrays)
    words = raw[4 * R.SUMMARY_WORDS:].view(np.uint32)
    wpr = (dims[0] + 31) // 32
    assert words.size == wpr * dims[1] * dims[2]
    rows = np.unpackbits(words.reshape(dims[2], dims[1], wpr).view(np.uint8), axis=-1, bitorder="little")
    assert not rows[:, :, dims[0]:].any()  # the padding bits
    return {"bits": rows[:, :, :dims[0]].astype(bool).transpose(2, 1, 0), "summary": R.summary_from_words(raw[:4 * R.SUMMARY_WORDS].copy()),
            "words": words}


def _assert_harness(harness, tmp_path, world, factor, origin, dims, rule, mask=None):
    want = R.apply_rule(world, origin, dims, rule, mask)
    got = _run_harness(harness, tmp_path, world, factor, origin, dims, rule, mask)
    assert np.array_equal(got["bits"], want["bits"]), (origin, dims, rule)
    assert got["summary"] == want["summary"], (origin, dims, rule)
    return got


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    for case in RC.all_cases():
        got = _assert_harness(harness, tmp_path, case["world"], 8, case["origin"], case["dims"], case["rule"], case["mask"])
        RC.check(case, got, got["words"])


def test_host_code_uses_every_mux_tree_leaf(harness, tmp_path):
    """the gradient cases, in which every pair (self, count) decides some free voxel (asserted above on the reference alone)"""
    for w, o, d, rule, mask in RC.gradient_cases():
        _assert_harness(harness, tmp_path, w, 8, o, d, rule, mask)


@pytest.mark.parametrize("nb", NEIGHBOURHOODS)
def test_host_code_at_every_halo_row_width(harness, tmp_path, nb):
    """halo rows of 31, 32, 33, 64, 65 and 96 voxels (one, two and three words), both scopes, 1, 2 and 16 iterations, both
    `outside` values, origins negative, unaligned and past the far faces; BOX with and without a mask"""
    rng = np.random.default_rng(100 + nb)
    w = R.gradient_world(rng)
    for halo_width in (31, 32, 33, 64, 65, 96):
        for scope, n in ((R.BOX, 1), (R.BOX, 2), (R.BOX, 16), (R.WORLD, 1), (R.WORLD, 2), (R.WORLD, 16)):
            h = n if scope == R.WORLD else 1
            d0 = halo_width - 2 * h
            if d0 < 1:
                continue
            for _ in range(50):  # a case is kept when, by the reference, voxels are born and die in it
                d = (d0, int(rng.integers(3, 7)), int(rng.integers(3, 7)))
                o = (int(rng.integers(-8, 64 - d0 // 2)), int(rng.integers(-3, 62)), int(rng.integers(-3, 62)))
                rule = R.random_rule(rng, nb, n, scope, int(rng.integers(0, 2)))
                mask = rng.random(d) < 0.75 if scope == R.BOX and n == 2 else None
                s = R.apply_rule(w, o, d, rule, mask)["summary"]
                if s[2] > 0 and s[3] > 0:
                    break
            assert s[2] > 0 and s[3] > 0
            _assert_harness(harness, tmp_path, w, 8, o, d, rule, mask)


@pytest.mark.parametrize("factor,edge", [(8, 64), (16, 128), (32, 256)])
def test_host_code_at_every_brick_edge(harness, tmp_path, factor, edge):
    rng = np.random.default_rng(factor)
    w = R.gradient_world(rng, (edge, edge, edge))
    for i, (o, d) in enumerate([((-7, edge // 2, -3), (40, 6, 5)), ((edge - 20, 3, edge - 4), (33, 5, 7)), ((edge + 4, 0, 0), (3, 3, 3))]):
        rule = R.random_rule(rng, NEIGHBOURHOODS[i], 2, i % 2, i % 2)
        got = _assert_harness(harness, tmp_path, w, factor, o, d, rule)
        assert (got["summary"][2] > 0 and got["summary"][3] > 0) == (i < 2)  # (the last box lies wholly outside the world)


def _layout(harness, tmp_path, origin, dims, rule):
    fields = np.asarray([rule.neighbours, rule.born, rule.survive, rule.iterations, rule.scope, rule.outside], np.int64)
    header = [1, 8, 64, 64, 64, *origin, *dims, *fields.astype(np.uint32).view(np.int32), 0]
    raw, _ = run_harness_files(harness, tmp_path, header)
    code, with_o, without = (int(v) for v in np.frombuffer(raw[:12].tobytes(), np.uint32))
    return code, bool(with_o), bool(without), int(np.frombuffer(raw[12:20].tobytes(), np.uint64)[0])


def test_argument_limits_without_a_device(tmp_path_factory):
    run_harness(build_harness(tmp_path_factory, "rule_args_check"))


def _expect_bytes(d, h):  # the formula of include/vxrt.h
    r = lambda n: (n + 255) // 256 * 256
    hd = [v + 2 * h for v in d]
    return 4 * r(4 * ((hd[0] + 31) // 32) * hd[1] * hd[2])


def test_rule_symbols_exported_and_workspace_bytes(harness, tmp_path):
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_rule_workspace_bytes", "vxrt_apply_rule", "vxrt_apply_rule_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    assert (vx.RULE_N6, vx.RULE_N18, vx.RULE_N26, vx.RULE_BOX, vx.RULE_WORLD, vx.RULE_MAX_ITERATIONS) == (R.N6, R.N18, R.N26, R.BOX, R.WORLD, 16)
    assert C.sizeof(vx.RuleDesc) == 32

    def ws(d, rule):
        desc = rule._c()
        return int(lib.vxrt_rule_workspace_bytes((C.c_int32 * 3)(*d), C.byref(desc)))

    box, world16 = vx.Rule.smooth(2), vx.Rule.smooth(16, scope=vx.RULE_WORLD)
    for bad in [(0, 8, 8), (8, -1, 8), (1 << 10, 1 << 10, (1 << 8) + 1), (1 << 29, 1, 1)]:
        assert ws(bad, box) == 0
    for bad in (vx.Rule(3, 1, 1), vx.Rule(vx.RULE_N6, 1 << 7, 0), vx.Rule(vx.RULE_N18, 0, 1 << 19), vx.Rule(vx.RULE_N26, 1 << 27, 0),
                vx.Rule(vx.RULE_N26, 1, 1, 0), vx.Rule(vx.RULE_N26, 1, 1, 17), vx.Rule(vx.RULE_N26, 1, 1, 1, 2),
                vx.Rule(vx.RULE_N26, 1, 1, 1, 0, 2), vx.Rule(vx.RULE_N26, 1 << 40, 1)):
        assert ws((8, 8, 8), bad) == 0, bad
    assert ws((1, 1, 1 << 28), box) > 0 and ws((1, 1, 1 << 28), world16) == 0  # the halo box against 2^36 voxels
    assert lib.vxrt_rule_workspace_bytes(None, C.byref(box._c())) == 0
    assert lib.vxrt_rule_workspace_bytes((C.c_int32 * 3)(8, 8, 8), None) == 0
    short = box._c()
    short.struct_size = 28
    assert lib.vxrt_rule_workspace_bytes((C.c_int32 * 3)(8, 8, 8), C.byref(short)) == 0
    for d in [(1, 1, 1), (30, 7, 5), (31, 3, 9), (33, 2, 2), (62, 64, 8), (100, 9, 3), (256, 128, 256), (1024, 256, 1024)]:
        for rule, h in ((box, 1), (world16, 16), (vx.Rule.grow(vx.RULE_N6, 3, scope=vx.RULE_WORLD), 3)):
            want = _expect_bytes(d, h)
            assert ws(d, rule) == want, (d, h)
            if d[0] <= 100:
                ref = R.RefRule(rule.neighbours, rule.born, rule.survive, rule.iterations, rule.scope, rule.outside)
                assert _layout(harness, tmp_path, (0, 0, 0), d, ref) == (0, True, True, want)
    assert ws((256, 128, 256), box) <= 256 * 128 * 256 * 5 // 8  # four bit planes of a halo barely larger than the box
    o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    assert lib.vxrt_apply_rule(None, o3, d3, None, None, None, None, None, None) == -1
    assert lib.vxrt_apply_rule_host(None, o3, d3, None, None, None, None) == -1


def test_the_python_rules_are_the_references():
    import voxelengine_amd as vx
    as_ref = lambda r: R.RefRule(r.neighbours, r.born, r.survive, r.iterations, r.scope, r.outside)
    assert as_ref(vx.Rule.smooth(3)) == R.smooth(3)
    for nb in NEIGHBOURHOODS:
        assert as_ref(vx.Rule.grow(nb)) == R.grow(nb) and as_ref(vx.Rule.erode(nb)) == R.erode(nb)
    assert as_ref(vx.Rule.caves(14, 13, 4)) == R.smooth(4)
    assert vx.Rule(vx.RULE_N6, (1, 2), [0, 6]).born == 0b110 and vx.Rule(vx.RULE_N6, (1, 2), [0, 6]).survive == 0b1000001
    assert vx.Rule.smooth().scope == vx.RULE_BOX and vx.Rule.smooth(scope=vx.RULE_WORLD, outside=1).outside == 1
