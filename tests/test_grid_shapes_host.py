"""The grid-shape cases of tests/grid_shape_cases.py held to what they claim, without a GPU: the sparse table builder
against the oracle's own, every case against the restated grid_is_wide under the constants read from the sources (and
under each of them moved by one step of 8 cells: a changed constant fails here instead of leaving the GPU test short of its
path), and the coverage of every case's rays, counted on the oracle's results alone."""
import re
import subprocess

import numpy as np
import pytest

from tests import grid_shape_cases as G
from tests import sparse_world
from tests.test_host_wave_logic import harness  # noqa: F401  (the fixture that builds tests/tools/host_wave_check.cpp)


@pytest.mark.parametrize("factor", [8, 16, 32])
@pytest.mark.parametrize("cells", [(8, 16, 24), (24, 8, 16), (16, 24, 8), (8, 8, 8)])
def test_tables_from_voxels_equal_the_oracles_builder(vxo, factor, cells):
    """bit-equal to World.from_voxels on grids with three different dimensions: coarse bits, slots, bounds (empty cells'
    included) and pool; single voxels (some twice), boxes across brick borders, a full brick, and empty cells in between"""
    rng = np.random.default_rng(factor + cells[0] * 3 + cells[1])
    dims = np.array(cells) * factor
    v = np.zeros(tuple(dims), bool)
    single = (rng.random((400, 3)) * dims).astype(np.int64)
    size = rng.integers(1, factor + 3, size=(12, 3))
    lo = (rng.random((12, 3)) * (dims - size)).astype(np.int64)
    full = np.array([[factor, 2 * factor, 3 * factor]])
    coords = np.concatenate([single, single[:50], sparse_world.voxels_of_boxes(lo, size),
                             sparse_world.voxels_of_boxes(full, [[factor] * 3])])
    v[coords[:, 0], coords[:, 1], coords[:, 2]] = True
    w = vxo.World.from_voxels(v, factor)
    assert w.cdims == tuple(cells)
    coarse, slot, bounds, pool = sparse_world.tables_from_voxels(coords, cells, factor)
    assert 0 < w.nslots < w.ncells
    assert coarse.dtype == np.uint32 and slot.dtype == np.uint32 and bounds.dtype == np.float32 and pool.dtype == np.uint32
    assert np.array_equal(coarse, w.coarse_bits)
    assert np.array_equal(slot, w.brick_slot)
    assert np.array_equal(bounds.view(np.uint32), w.bounds.view(np.uint32))
    assert np.array_equal(pool, w.pool)
    # ... and no voxel at all
    coarse, slot, bounds, pool = sparse_world.tables_from_voxels(np.zeros((0, 3), np.int64), cells, factor)
    assert not coarse.any() and (slot == sparse_world.EMPTY_SLOT).all() and len(pool) == 0
    assert (bounds == np.array([0, 0, 0, -1, -1, -1], np.float32)).all()


def test_every_case_is_on_its_side_of_the_predicate():
    caps = G.read_caps()
    assert caps["max_steps"] == 2048    # MAX_STEPS of the reference
    for case in G.CASES:
        assert G.check_case(case, caps) == [], case
    # every disjunct is reached alone by some case, and both sides of every cap are taken
    assert {c.disjunct for c in G.CASES if c.alone} >= {"y", "z", "sum"}
    assert sum(c.side == "ordinary" for c in G.CASES) >= 6


@pytest.mark.parametrize("name", list(G.CAP_SOURCES))
@pytest.mark.parametrize("step", [8, -8])
def test_a_constant_moved_by_eight_cells_flips_a_case(name, step):
    caps = G.read_caps()
    caps[name] += step
    assert [why for case in G.CASES for why in G.check_case(case, caps)], (name, step)


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_rays_of_every_case_cover_what_they_are_for(vxo, name):
    """the coverage conditions, on World.wrap(...).trace_batch: per long axis and direction walks of 0.9 x the cells (at
    most 2047) and misses that leave through the far face; walks that end by MAX_STEPS where an axis has 2048 cells; hits
    after more than 400 steps; far-face starts that hit"""
    case = G.BY_NAME[name]
    assert case.long_axes
    w = G.world(vxo, case)
    o, d, group = G.rays(case, G.N_RAYS, case.seed)
    # the families keep to their description: on the far face exactly, 3 voxels outside, on integer cross coordinates
    for gi, (fam, ax, sg) in enumerate(G.ray_groups(case)):
        m = group == gi
        assert m.sum() >= G.N_RAYS // 2 // len(G.ray_groups(case))
        if fam == "far_face":
            assert (o[m, ax] == (0.0 if sg > 0 else case.dims[ax])).all() and (np.sign(d[m, ax]) == sg).all()
        elif fam == "outside":
            assert (o[m, ax] == (-3.0 if sg > 0 else case.dims[ax] + 3.0)).all()
        elif fam == "parallel":
            cross = [a for a in range(3) if a != ax]
            assert (d[m][:, cross] == 0).all() and (o[m][:, cross] == np.floor(o[m][:, cross])).all()
    res = w.trace_batch(o, d, nthreads=16)
    cov = G.coverage(case, o, d, group, res)
    assert G.coverage_shortfalls(case, cov) == [], cov
    assert 0 < int(res["hit"].sum()) < len(o)
    if case.ncells * case.factor ** 3 > 1 << 32:
        assert int(res["voxel"].max()) > 1 << 32      # voxel indices beyond 32 bits are in the comparison


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_rays_of_every_case_through_the_tracer_on_the_host(vxo, harness, tmp_path, name):  # noqa: F811
    """Every case's own tables and rays through the product's per-lane code on the CPU (tests/tools/host_wave_check.cpp reads
    them from a file): the wave tracer with one lane per wave, the persistent lane and the straightforward loops against the
    oracle, ray by ray, on arrays padded with exactly the slack the allocator promises and with the load guard counting.
    This is where the cases that no dense array holds (two long axes, the sum disjunct, 65528 cells) meet the tracer without
    a GPU."""
    case = G.BY_NAME[name]
    coarse, slot, bounds, pool = G.tables(name)
    o, d, _ = G.rays(case, G.N_RAYS, case.seed)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([case.factor, *case.cells, len(pool) // (case.factor ** 3 // 32), len(o)], np.int32).tobytes())
        for a in (coarse, slot, bounds, pool, o, d):
            f.write(np.ascontiguousarray(a).data)
    out = subprocess.run([harness, "@" + str(path)], capture_output=True, text=True)
    path.unlink()
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:])
    assert "mismatches 0 of %d" % len(o) in out.stdout and "outside it 0)" in out.stdout and "UNSUSPECTED EXITS" not in out.stdout, out.stdout[-2000:]
    exhausted = int(re.search(r"without a hit (\d+)", out.stdout).group(1))
    if max(case.cells) >= 2048:
        assert exhausted >= 100, out.stdout
