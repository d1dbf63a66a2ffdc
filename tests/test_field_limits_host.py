"""The field limit cases (tests/field_limit_cases.py) without a GPU: the launch caps read from the sources, every case past
the cap it targets, a copy of the sources with any one cap raised 64-fold leaving some case short (so raising a cap fails
here instead of quietly emptying tests/test_gpu_field_limits.py), the constructions of the GPU cases held to what they
promise (emitter classes per workgroup, levels past the first tally pass, result rows no shift maps onto themselves), the
closed forms held against the restatements (tests/ref_light.py) at small sizes, and the 65536-entry emitter list, the tall
world and scaled-down twins of the piece batches through the kernels' code on the host (tests/tools/light_check.cpp,
tests/tools/place_check.cpp), with the store width of the light output at every address residue
(tests/tools/light_args_check.cpp)."""
import os
import re

import numpy as np
import pytest

from tests import field_limit_cases as F
from tests import ref_light as RL
from tests import ref_place as RP
from tests.helpers import build_harness, run_harness
from tests.test_light_host import _assert_harness as _light_harness
from tests.test_place_host import _pack, _run_harness as _place_harness, classes


def _short(caps):
    return [(case.name, what, value, bound) for case in F.LAUNCH_CASES for what, value, bound in case.reach(caps)
            if not value > bound]


# ---- the caps --------------------------------------------------------------------------------------------------------------
def test_caps_are_read_from_the_sources():
    c = F.read_caps()
    assert all(v > 0 for v in c.values())
    assert (c["light_halo"], c["light_max_emitters"]) == (RL.HALO, RL.MAX_EMITTERS)
    assert (c["place_max_dim"], c["place_max_voxels"]) == (RP.MAX_DIM, RP.MAX_VOXELS)
    assert F.SHEET_EDGE ** 2 <= c["place_max_voxels"]  # the sheet is within the contract
    assert F.place_shape(F.table_shapes(F.SHEET_EDGE)) == (64, 16384) and F.place_most(F.table_shapes(F.SHEET_EDGE), c) == 1024
    assert F.place_shape([(1, 1, 1)]) == (1, 1)
    assert F.tally_groups(F.STRIDE_DIMS, c) == (157, 128) and F.tally_groups(F.CAP_DIMS, c) == (8327, 1024)


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


# ---- light: harness, constructions, closed forms ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def light_check(tmp_path_factory):
    return build_harness(tmp_path_factory, "light_check")


def _same(a, b):
    return np.array_equal(a["levels"], b["levels"]) and a["summary"] == b["summary"]


def test_single_channel_fields_from_the_two_channel_one():
    rng = np.random.default_rng(3)
    w = RL.leaky_roof_world(rng)
    o, d = (3, 20, 2), (20, 17, 19)
    e = [(10, 30, 10, 15), (12, 25, 9, 7), (200, 0, 0, 3), (5, 5, 5, 0)] + [(*(int(v) for v in rng.integers(0, 40, 3)), 12) for _ in range(9)]
    both = RL.light_field(w, o, d, e)
    assert min(both["summary"][6:10]) > 0 and both["summary"][1] > 0
    for channels in F.MASKS:
        assert _same(F.single_channel(both, channels), RL.light_field(w, o, d, e, channels)), channels


def test_the_emitter_list_is_what_the_case_promises(light_check, tmp_path):
    caps = F.read_caps()
    lanes = caps["classify_lanes"]
    e, cls, shared, special = F.emitter_list()
    world, o, d = F.emitter_world(), F.EM_ORIGIN, F.EM_DIMS
    assert e.shape == (caps["light_max_emitters"], 4) and len(set(special + [shared])) == len(F.EM_SPECIAL) + 1
    per_block = np.stack([np.bincount(cls[b:b + lanes], minlength=4) for b in range(0, len(cls), lanes)])
    assert (per_block[:, 0] > 0).all() and (per_block[1:] > 0).all()  # a used one in every block; every class past the first
    assert (cls[list(F.EM_SPECIAL)] == 0).all() and [tuple(r[:3]) for r in e[list(F.EM_SPECIAL)]] == special
    on_shared = np.flatnonzero((e[:, :3] == shared).all(1) & (cls == 0))
    assert len(on_shared) >= 4096 and len(set(on_shared // lanes)) == len(cls) // lanes
    assert set(e[on_shared, 3].tolist()) == set(range(1, 16)) and e[on_shared[0], 3] < 15   # the maximum is not the first
    run = e[F.EM_ROW_STEP * np.arange(64) + F.EM_ROW_AT]
    hx = run[:, 0] - (o[0] - caps["light_halo"])
    assert sorted((hx >> 5).tolist()) == [1] * 32 + [2] * 32 and len(set(hx.tolist())) == 64  # every bit of two neighbouring words
    for n in F.EM_COUNTS:
        want = F.emitter_reference(n)
        assert want["summary"][6:10] == tuple(np.bincount(cls[:n], minlength=4)), n   # the classes by construction are the classes
        assert all(v > 0 for v in want["summary"][3]), n                                # every block level occurs
        blk = want["levels"] & 15
        at = lambda p: int(blk[p[0] - o[0], p[1] - o[1], p[2] - o[2]])
        assert at(shared) == 15
        assert (blk[run[:, 0] - o[0], F.EM_ROW[1] - o[1], F.EM_ROW[2] - o[2]] == (F.EM_ROW_STEP * np.arange(64) + F.EM_ROW_AT < n)).all()
        for k, (i, p) in enumerate(zip(F.EM_SPECIAL, special)):
            assert i >= n or at(p) >= 9 + k, (n, i)
    # what an entry adds shows in the field: the lists of 256 and 257 entries differ by the used emitter 256 alone
    a, b = F.emitter_reference(256), F.emitter_reference(257)
    assert b["summary"][6] == a["summary"][6] + 1 and not np.array_equal(a["levels"], b["levels"])
    assert not np.array_equal(b["levels"], F.emitter_reference(65536)["levels"])
    got = _light_harness(light_check, tmp_path, np.asarray(world), 8, o, d, e, RL.SKY | RL.BLOCK)
    assert _same(got, F.emitter_reference(65536))


def test_the_stride_case_has_every_level_past_the_first_pass():
    caps = F.read_caps()
    want = F.stride_reference()
    past = F.tally_word_index(F.STRIDE_DIMS, caps) >= F.tally_groups(F.STRIDE_DIMS, caps)[1] * 256
    solid = F.box_solid(F.stride_world(), F.STRIDE_ORIGIN, F.STRIDE_DIMS)
    sky, block = F.levels_at(want["levels"], solid, past)
    assert sky == set(range(16)) and block == set(range(16))
    assert past.any() and not past.all() and want["summary"][6] == len(F.stride_emitters())


@pytest.mark.parametrize("origin,dims", [((20, -50, -18), (1, 100, 100)), ((-13, -10, -12), (90, 40, 90)), ((20, 60, 30), (3, 9, 2)),
                                         ((-3, -60, 20), (5, 4, 3)), ((20, -60, 20), (5, 4, 3))])
def test_cube_sky_equals_the_restatements(origin, dims):
    want = F.cube_field(origin, dims)
    for channels in (RL.SKY | RL.BLOCK, RL.SKY):
        assert _same(F.single_channel(want, channels), RL.light_field(F.cube_world(), origin, dims, None, channels))
    assert _same(want, RL.light_field_relax(F.cube_world(), origin, dims))
    if dims[0] == 1 and dims[1] == 100:
        assert set((want["levels"] >> 4).ravel().tolist()) == set(range(16))  # at x = 20 every level occurs


def test_the_cap_case_has_every_level_past_the_first_pass():
    caps = F.read_caps()
    sky, solid, exposed = F.cube_sky(F.CAP_ORIGIN, F.CAP_DIMS)
    past = F.tally_word_index(F.CAP_DIMS, caps) >= caps["tally_max"] * 256
    assert set(sky[past & ~solid].tolist()) == set(range(16)) and solid[past].sum() == solid.sum() == 64 * 64
    assert set(sky[~past].tolist()) == {15}  # all of it past the first pass


def test_cube_and_lamps_closed_form_equals_the_restatement():
    o, d = (-36, -34, -35), (132, 130, 131)
    lamps, counts = F.open_air_lamps(o, d, 12, 7)
    want = RL.light_field(F.cube_world(), o, d, lamps)
    assert want["summary"][6:10] == counts and want["summary"][0] == 64 ** 3
    for slab in (F.MAXV_SLAB, 7):
        assert _same(F.cube_lamps_field(o, d, lamps, counts, slab), want), slab
    assert sum(want["summary"][3][1:]) > 1000 and min(want["summary"][2]) > 0


def test_the_tall_world_columns_and_the_clamp_on_the_host_code(light_check, tmp_path):
    caps = F.read_caps()
    world, o, d = F.tall_world(caps), F.ABOVE_ORIGIN, F.ABOVE_DIMS
    want = RL.light_field(world, o, d, None, RL.SKY)
    sky = want["levels"] >> 4
    hand = np.full(d, 15)
    for x, z in F.ABOVE_COLUMNS:
        hand[x - o[0], :, z - o[2]] = 14
    assert np.array_equal(sky, hand) and world.sum() == 64 * 4 * 64 + 4
    assert _same(_light_harness(light_check, tmp_path, world, 8, o, d, None, RL.SKY), want)
    for co, cd in F.CLAMP_BOXES:
        assert F.above_first(co, cd, caps) == 0 and co[1] + cd[1] + caps["light_halo"] < 0
        assert _same(_light_harness(light_check, tmp_path, F.cube_world(), 8, co, cd, None, RL.SKY | RL.BLOCK), F.cube_field(co, cd))
    assert len(set((F.cube_field(*F.CLAMP_BOXES[1])["levels"] >> 4).ravel().tolist())) > 2


def test_the_store_width_follows_the_output_address(tmp_path_factory):
    """light_args clears `wide` off the dword grid, and the byte stores give the dword stores' bytes (the device stores
    misaligned dwords without complaint, so only the host code can tell whether the flag follows the address)"""
    with open(os.path.join(F.ROOT, "tests", "tools", "light_args_check.cpp")) as f:
        line = re.search(r"boxes\[5\]\[3\] = (.*);", f.read()).group(1)
    boxes = [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", line)]
    assert boxes == [d for _, d in F.UNALIGNED_BOXES]
    out = run_harness(build_harness(tmp_path_factory, "light_args_check"))
    assert " 0 lanes" not in out and "failures 0" in out


# ---- pieces: the twins through the host code -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def place_check(tmp_path_factory):
    return build_harness(tmp_path_factory, "place_check")


def _twin(place_check, tmp_path, pieces, pl):
    vox = np.asarray(F.piece_world())
    a, b = RP.place(vox, pieces, pl, RP.place_shift), F.sheet_reference(vox, pieces, pl)
    assert np.array_equal(a, b)
    got, out = _place_harness(place_check, tmp_path, vox, F.PIECE_WORLD[3], [_pack(p) for p in pieces], [p.shape for p in pieces], pl)
    assert np.array_equal(got, RP.pack_results(a)), np.flatnonzero((got != RP.pack_results(a)).any(1))[:10]
    return a, out


def _assert_sheets(want, sheets):
    """the sheet placements in turn: a fit that overlaps, a drop that lands after moving, a sweep that is stopped"""
    for k, i in enumerate(sheets):
        if k % 3 == 0:
            assert want[i, 0] > 3 and want[i, 3] == 0, (i, want[i])
        else:
            assert want[i, 3] == RP.BLOCKED and want[i, 1] != 0 and want[i, 2] > 0, (i, want[i])


def test_grid_y_twin(place_check, tmp_path):
    edge = F.SHEET_EDGE_TWIN
    pieces = F.piece_table(edge)
    assert pieces[0][0, edge - 1, edge - 1] and pieces[0].shape == (1, edge, edge) and F.place_shape([p.shape for p in pieces]) == (64, 16)
    want, out = _twin(place_check, tmp_path, pieces, F.grid_y_batch(edge))
    assert "lanes 64, tasks 16" in out
    _assert_sheets(want, F.GRID_Y_SHEETS)
    assert min(classes(want)) > 0


def _assert_cut(pl, cuts, want, most):
    n = len(pl)
    assert n == 2 * most + 7 and cuts.tolist() == [most - 1, most, 2 * most - 1, 2 * most]
    assert (want[cuts, 3] == RP.BLOCKED).all()
    assert (want[1:] != want[:-1]).any(1).all()                     # every row differs from its neighbours
    assert F.no_shift_maps_onto_itself(want) and F.no_shift_maps_onto_itself(pl)
    assert F.no_shift_maps_onto_itself(want, most) and F.no_shift_maps_onto_itself(want, 2 * most)
    invalid = np.flatnonzero(want[:, 3] == RP.INVALID)
    assert len(invalid) == 4 and {int(i) // most for i in invalid} == {0, 1, 2}
    sheets = np.flatnonzero(pl[:, 0] == 0)
    assert [int(i) // most for i in sheets] == [0, 1, 2]
    _assert_sheets(want, sheets)
    assert all(want[most * k:most * (k + 1), 3].any() and want[most * k:most * (k + 1), 1].any() for k in range(3))


def test_batch_cut_twin(place_check, tmp_path):
    edge, most = F.SHEET_EDGE_TWIN, F.CUT_MOST_TWIN
    pl, cuts = F.cut_batch(edge, most)
    want, _ = _twin(place_check, tmp_path, F.piece_table(edge), pl)
    _assert_cut(pl, cuts, want, most)
    assert not F.no_shift_maps_onto_itself(np.tile(want[:5], (3, 1)))  # the property can fail


def test_init_stride_base(place_check, tmp_path):
    pl = F.init_base()
    one = [np.ones((1, 1, 1), bool)]
    vox = np.asarray(F.piece_world())
    want = RP.place(vox, one, pl)
    assert np.array_equal(want, RP.place(vox, one, pl, RP.place_shift))
    got, out = _place_harness(place_check, tmp_path, vox, F.PIECE_WORLD[3], [_pack(one[0])], [(1, 1, 1)], pl)
    assert np.array_equal(got, RP.pack_results(want)) and "lanes 1, tasks 1" in out
    assert len(pl) == F.INIT_BASE and min(classes(want)) > 0 and np.count_nonzero(want[:, 3] == RP.INVALID) > 40
    assert want[1].tolist() == [0, 0, 1, 1] and want[2].tolist() == [0, -8, 1, 1] and want[3].tolist() == [0, 12, 0, 0] and want[4, 0] == 1
    # the placements of the second pass of the grid-stride loop: not all alike
    tail = (F.read_caps()["place_blocks"] * 256 + np.arange(F.INIT_EXTRA)) % F.INIT_BASE
    assert len({tuple(r) for r in want[tail].tolist()}) > 5 and (want[tail, 3] == RP.INVALID).any() and (want[tail, 3] == RP.BLOCKED).any()
