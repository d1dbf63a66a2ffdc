"""CPU checks of the loose voxels (include/vxrt.h, vxrt_loose_step): the two restatements of tests/ref_loose.py against each
other and on the hand-derived cases of tests/loose_cases.py, their invariants on random scenes (mass, blocked voxels, targets,
steps across calls, translation), sand coming to rest, and the kernels' per-lane code (csrc/vxrt_loose.hpp) compiled for the
host (tests/tools/loose_check.cpp) against them -- layer and summary bit-equal, every index checked, with and without the
zero-stencil shortcut, in place and out of place, once under ASan and UBSan -- with the workspace formula, the limits of the
arguments and the refusal order of the parameters (tests/tools/loose_args_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import loose_cases as LC
from tests import ref_loose as R
from tests import helpers
from tests.helpers import build_harness, run_harness, run_harness_files


def _same(a, b, what):
    assert np.array_equal(a["bits"], b["bits"]) and a["summary"] == b["summary"], (what, a["summary"], b["summary"])


def _both(case):
    a = LC.run(R.loose_step, case)
    _same(a, LC.run(R.loose_step_sets, case), case["name"])
    return a


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def test_hand_derived_cases_on_the_restatements():
    names = set()
    for case in LC.hand_cases():
        LC.check(case, _both(case))
        names.add(case["name"])
    assert {"fall3", "column_sand", "column_water", "drain2", "ledge_taken", "dropped", "spread_x31_t0", "slide_x32_t2", "phase3", "wrap"} <= names


def test_the_restatements_agree_on_random_scenes():
    moved = drained = 0
    for seed in (0, 1):
        for case in LC.random_cases(seed):
            s = _both(case)["summary"]
            moved += s[3] + s[4] + s[5]
            drained += s[1] - s[2]
            assert case["edge"] == R.OPEN or s[1] == s[2]
    assert moved > 100 and drained > 10


def test_mass_blocked_voxels_and_targets():
    """|L| + drained is constant; L never meets a blocked voxel and stays in Live; within a pass no two movers share a target
    (asserted inside loose_step_sets for every pass) and every mover's target was free"""
    for case in LC.random_cases(3):
        r = R.loose_step_sets(case["world"], case["origin"], case["dims"], case["loose"], case["material"], case["steps"], case["edge"],
                              case["phase"], keep_passes=True)
        s = r["summary"]
        assert s[2] + r["drained"] == s[1]
        assert len(r["passes"]) == case["steps"] * len(R.passes_of(case["material"]))
        for t, kind, moves in r["passes"]:
            assert len({m[1] for m in moves}) == len(moves) and all(abs(a - b) <= 1 for m in moves for a, b in zip(*m))
        w, inw = R._halo(case["world"], case["origin"], case["dims"])
        box = tuple(slice(1, 1 + n) for n in case["dims"])
        assert not (r["bits"] & (w[box] | ~inw[box])).any()


def test_n_steps_are_n_single_steps_with_the_phase_advanced():
    for case in LC.random_cases(5, 8):
        whole = LC.run(R.loose_step, case)
        cur, first = case["loose"], None
        for i in range(case["steps"]):
            step = R.loose_step(case["world"], case["origin"], case["dims"], cur, case["material"], 1, case["edge"], case["phase"] + i)
            first = first or step
            cur = step["bits"]
        assert np.array_equal(whole["bits"], cur) and whole["summary"][2:6] == step["summary"][2:6]
        assert whole["summary"][:2] == first["summary"][:2]
        # only phase & 3 matters
        _same(whole, R.loose_step(case["world"], case["origin"], case["dims"], case["loose"], case["material"], case["steps"], case["edge"],
                                  case["phase"] & 3), case["name"])


def test_translation_by_an_even_offset_translates_the_result():
    """world, box and layer moved by an even offset along every axis: the same layer, the changed box moved with it (the
    directions depend on coordinate parities alone)"""
    rng = np.random.default_rng(7)
    shape = (20, 12, 16)
    odd_differs = moved_total = 0
    for i in range(8):
        world = R.terrain(rng, shape, 1, 5, 0.15)
        # the box and one voxel around it inside the world, so that the moved world has the same voxels around the moved box
        o = tuple(int(rng.integers(1, s - 4)) for s in shape)
        d = tuple(int(rng.integers(1, s - a)) for s, a in zip(shape, o))
        layer = R.random_layer(rng, d, 0.3)
        args = (i & 1, 1 + i % 5, (i >> 1) & 1, i)
        a = R.loose_step(world, o, d, layer, *args)
        moved_total += a["summary"][3] + a["summary"][4] + a["summary"][5]
        for off in [tuple(int(v) * 2 for v in rng.integers(0, 4, 3)), (1, 0, 0)]:
            moved = np.zeros(tuple(s + k for s, k in zip(shape, off)), bool)
            moved[off[0]:, off[1]:, off[2]:] = world
            b = R.loose_step(moved, tuple(v + k for v, k in zip(o, off)), d, layer, *args)
            if off == (1, 0, 0):  # an odd offset is another rule: counted, not asserted per case
                odd_differs += int(not np.array_equal(a["bits"], b["bits"]))
                continue
            assert np.array_equal(a["bits"], b["bits"]) and a["summary"][:6] == b["summary"][:6]
            if a["summary"][6] == R.NONE[0]:
                assert b["summary"][6:] == R.NONE
                continue
            assert tuple(v + k for v, k in zip(a["summary"][6], off)) == b["summary"][6]
            assert tuple(v + k for v, k in zip(a["summary"][7], off)) == b["summary"][7]
    assert odd_differs > 0 and moved_total > 50


@pytest.mark.parametrize("edge,n", [(16, 256), (24, 768)])
def test_sand_comes_to_rest(edge, n):
    """a walled box over random 1 .. 4-high terrain: stepped until fell = slid = 0 in four steps running, one of each
    phase & 3, within 256 steps (a condition on the scenes chosen); then no loose voxel has a free voxel below or an open slide
    in either direction of either axis.  (One quiet step is not enough: a step offers every voxel one direction only, and a
    voxel whose slide is open the other way waits for the step that offers it; include/vxrt.h says so.)"""
    rng = np.random.default_rng(edge)
    world = R.terrain(rng, (edge, edge, edge), 1, 4)
    layer = np.zeros((edge, edge, edge), bool)
    free = np.argwhere(~world[:, : edge // 2, :])
    pick = free[rng.choice(len(free), n, replace=False)]
    layer[pick[:, 0], pick[:, 1], pick[:, 2]] = True
    box = ((0, 0, 0), (edge, edge, edge))
    steps, quiet = None, 0
    for t in range(256):
        r = R.loose_step(world, *box, layer, R.SAND, 1, R.WALL, t)
        layer = r["bits"]
        quiet = quiet + 1 if r["summary"][3] == 0 and r["summary"][4] == 0 else 0
        if quiet == 4:
            steps = t + 1
            break
    assert steps is not None and int(layer.sum()) == n
    occupied = np.pad(world | layer, 1, constant_values=True)  # the walls
    c = slice(1, -1)
    below = occupied[c, :-2, c]
    assert not (layer & ~below).any()
    for side, under in ((occupied[2:, c, c], occupied[2:, :-2, c]), (occupied[:-2, c, c], occupied[:-2, :-2, c]),
                        (occupied[c, c, 2:], occupied[c, :-2, 2:]), (occupied[c, c, :-2], occupied[c, :-2, :-2])):
        assert not (layer & ~side & ~under).any()
    assert R.at_rest(world, *box, layer)
    # a further step of any number changes nothing: a fixed point
    for t in range(4):
        assert np.array_equal(R.loose_step(world, *box, layer, R.SAND, 1, R.WALL, t)["bits"], layer)


# ---- the kernels' per-lane code on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "loose_check")


def _run_harness(exe, tmp_path, case, factor=8, shortcut=True, in_place=False):
    from oracle import vxo
    X, Y, Z = case["world"].shape
    d = case["dims"]
    header = [0, factor, X, Y, Z, *case["origin"], *d, case["material"], case["steps"], case["edge"], case["phase"], int(shortcut), int(in_place)]
    raw, _ = run_harness_files(exe, tmp_path, np.asarray(header, np.int64).astype(np.uint32).view(np.int32),
                               vxo.dense_from_voxels(case["world"]), LC.words_of(case))
    words = raw[4 * R.SUMMARY_WORDS:].view(np.uint32)
    wpr = (d[0] + 31) // 32
    assert words.size == wpr * d[1] * d[2]
    rows = np.unpackbits(words.reshape(d[2], d[1], wpr).view(np.uint8), axis=-1, bitorder="little")
    assert not rows[:, :, d[0]:].any()  # the padding bits
    return {"bits": rows[:, :, :d[0]].astype(bool).transpose(2, 1, 0), "summary": R.summary_from_words(raw[:4 * R.SUMMARY_WORDS].copy())}


def _assert_harness(exe, tmp_path, case, factor=8):
    want = LC.run(R.loose_step, case)
    for shortcut, in_place in ((True, False), (False, False), (True, True)):
        _same(_run_harness(exe, tmp_path, case, factor, shortcut, in_place), want, (case["name"], shortcut, in_place))
    return want


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    for case in LC.hand_cases():
        LC.check(case, _run_harness(harness, tmp_path, case))
        _assert_harness(harness, tmp_path, case)


def test_host_code_on_random_scenes(harness, tmp_path):
    for case in LC.random_cases(11, 10):
        _assert_harness(harness, tmp_path, case)


def _wide_case(rng, width, material, edge, steps, factor_edge=64):
    """a box `width` wide at a random place over the x faces of a leaky terrain world, densely filled"""
    world = R.terrain(rng, (factor_edge, 64, 64), 1, 5, 0.2)
    d = (width, int(rng.integers(3, 8)), int(rng.integers(3, 8)))
    o = (int(rng.integers(-3, max(factor_edge - width + 4, -2))), int(rng.integers(-1, 3)), int(rng.integers(-2, 10)))
    return dict(name="w%d" % width, world=world, origin=o, dims=d, loose=R.random_layer(rng, d, 0.35), material=material, steps=steps,
                edge=edge, phase=int(rng.integers(0, 4)), padding=True)


def test_host_code_at_every_halo_row_width(harness, tmp_path):
    """boxes 1, 29 .. 33 and 61 .. 65 wide (halo rows of 3, 31 .. 35 and 63 .. 67 bits: one, two and three words), both
    materials and edges, every phase & 3 over the cases"""
    rng = np.random.default_rng(21)
    moved = 0
    for i, width in enumerate((1, 29, 30, 31, 32, 33, 61, 62, 63, 64, 65)):
        for material in (R.SAND, R.WATER):
            s = _assert_harness(harness, tmp_path, _wide_case(rng, width, material, (i + material) & 1, 1 + i % 4))["summary"]
            moved += s[3] + s[4] + s[5]
    assert moved > 200


@pytest.mark.parametrize("factor,edge", [(8, 64), (16, 128), (32, 256)])
def test_host_code_at_every_brick_edge(harness, tmp_path, factor, edge):
    rng = np.random.default_rng(factor)
    world = R.terrain(rng, (edge, edge, edge), 1, 6, 0.1)
    for i, (o, d) in enumerate([((-7, 0, -3), (40, 9, 12)), ((edge - 20, 1, edge - 9), (33, 8, 14)), ((edge + 4, 0, 0), (3, 3, 3))]):
        case = dict(name="brick%d" % i, world=world, origin=o, dims=d, loose=R.random_layer(rng, d, 0.3), material=i & 1, steps=3, edge=i & 1,
                    phase=i, padding=False)
        s = _assert_harness(harness, tmp_path, case, factor)["summary"]
        assert (s[1] > 0) == (i < 2)  # (the last box lies wholly outside the world: everything is dropped)


def test_the_harness_under_sanitizers(tmp_path):
    """the harness's own main, stand-alone, under ASan and UBSan"""
    exe = str(tmp_path / "loose_check_san")
    root = helpers.ROOT
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(root, "tests", "tools", "hoststub"), "-I" + os.path.join(root, "oracle"), "-o", exe,
                        os.path.join(root, "tests", "tools", "loose_check.cpp"), "-x", "c",
                        *[os.path.join(root, "oracle", f) for f in ("vxo_trace.c", "vxo_world.c", "vxo_render.c")], "-lm", "-lpthread", "-w"],
                       capture_output=True, text=True)
    if r.returncode != 0 and any(s in r.stderr.lower() for s in ("sanitize", "asan", "ubsan")):
        pytest.skip("no sanitizer runtime for the host compiler")
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(2)
    for width, material in ((33, R.WATER), (64, R.SAND)):
        _assert_harness(exe, tmp_path, _wide_case(rng, width, material, R.OPEN, 3))


def test_argument_limits_without_a_device(tmp_path_factory):
    run_harness(build_harness(tmp_path_factory, "loose_args_check"))


def _expect_bytes(d):  # the formula of include/vxrt.h
    r = lambda n: (n + 255) // 256 * 256
    return 4 * r(4 * ((d[0] + 2 + 31) // 32) * (d[1] + 2) * (d[2] + 2))


def test_loose_symbols_exported_and_workspace_bytes():
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_loose_workspace_bytes", "vxrt_loose_step", "vxrt_loose_step_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    assert lib.vxrt_abi_version() == 3
    assert (vx.LOOSE_SAND, vx.LOOSE_WATER, vx.LOOSE_WALL, vx.LOOSE_OPEN, vx.LOOSE_MAX_STEPS) == (R.SAND, R.WATER, R.WALL, R.OPEN, R.MAX_STEPS)
    assert C.sizeof(vx.LooseDesc) == 32
    ws = lambda d: int(lib.vxrt_loose_workspace_bytes((C.c_int32 * 3)(*d)))
    for bad in [(0, 8, 8), (8, -1, 8), (1 << 10, 1 << 10, (1 << 8) + 1), (1 << 29, 1, 1)]:
        assert ws(bad) == 0
    assert lib.vxrt_loose_workspace_bytes(None) == 0
    for d in [(1, 1, 1), (30, 7, 5), (31, 3, 9), (33, 2, 2), (62, 64, 8), (100, 9, 3), (256, 128, 256), (1 << 14, 1, 1 << 14), (1, 1, 1 << 28)]:
        assert ws(d) == _expect_bytes(d), d
    assert ws((256, 128, 256)) <= 256 * 128 * 256 * 5 // 8  # four bit planes of a halo barely larger than the box
    o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    assert lib.vxrt_loose_step(None, o3, d3, None, None, None, None, None, None) == -1
    assert lib.vxrt_loose_step_host(None, o3, d3, None, None, None, None) == -1


def test_the_python_parameters():
    import voxelengine_amd as vx
    p = vx.Loose(vx.LOOSE_WATER, 7, vx.LOOSE_OPEN, 2 ** 32 + 5)._c()
    assert (p.struct_size, p.material, p.steps, p.edge, p.phase, tuple(p.reserved_)) == (32, 1, 7, 1, 5, (0, 0, 0))
    d = vx.Loose()
    assert (d.material, d.steps, d.edge, d.phase) == (vx.LOOSE_SAND, 1, vx.LOOSE_WALL, 0)
