"""The continuation hook of the wave tracer's end-of-walk phase (voxelengine_amd/csrc/vxrt_wave2.hpp:
phase_end_deferred<STATS, HOOK>) compiled for the HOST (tests/tools/host_end_hook_check.cpp): one persistent lane runs pairs
of rays through the two golden worlds in the order of a round of the render kernel; a first ray that ends on a voxel is
re-launched BY THE HOOK, inside the end-of-walk phase, along a fixed direction -- as the render kernel turns a primary hit
into its shadow ray -- unless the new start lies outside the coarse grid, in which case the ray-finished phase launches it.
Every second ray's result and probe counters equal those of begin_ray + the undeferred phases on a fresh tracer and the C
oracle's; every first ray's result, read by the hook, equals the oracle's."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
make_golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_golden)

INV = float(np.float32(1.0) / np.sqrt(np.float32(3.0)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return helpers.build_harness(tmp_path_factory, "host_end_hook_check")


@pytest.fixture(scope="module")
def worlds(vxo, tmp_path_factory):
    """the golden worlds (tests/golden/make_golden.py) as files of dense voxel words, checked against the golden tables"""
    d = tmp_path_factory.mktemp("hook_worlds")
    out = {}
    dense = helpers.gen_dense(vxo, vxo.GEN_INT_TERRAIN, 128, 128, 128)
    out["terrain"] = ((128, 128, 128, 16), dense, make_golden.world_terrain())
    vox = np.random.default_rng(77).random((64, 64, 64)) < 0.02  # helpers.random_voxel_world(vxo, (64, 64, 64), 8, 0.02, 77)
    out["sparse"] = ((64, 64, 64, 8), vxo.dense_from_voxels(vox), make_golden.world_sparse())
    paths = {}
    for name, (hdr, words, golden) in out.items():
        mine = vxo.World.from_dense(words, hdr[0], hdr[1], hdr[2], hdr[3])
        assert np.array_equal(mine.coarse_bits, golden.coarse_bits) and np.array_equal(mine.pool, golden.pool)
        paths[name] = str(d / (name + ".bin"))
        with open(paths[name], "wb") as f:
            f.write(np.asarray(hdr, np.int32).tobytes())
            f.write(np.ascontiguousarray(words, np.uint32).tobytes())
    return paths


def _run(exe, path, n, direction):
    out = subprocess.run([exe, path, str(n), *["%.9g" % v for v in direction]], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "mismatches 0 of %d" % n in out.stdout, out.stdout[-2000:]
    m = re.search(r"first hits (\d+); second rays launched by the hook (\d+), by the ray-finished phase (\d+); second rays that hit (\d+); "
                  r"direction special (\d); loads outside the tables' slack (\d+)", out.stdout)
    return [int(v) for v in m.groups()]


@pytest.mark.parametrize("world", ["terrain", "sparse"])
@pytest.mark.parametrize("direction", [(INV, INV, INV), (-0.3, 0.8, 0.52), (0.6, -0.2, -0.77)])
def test_second_ray_launched_by_the_hook_equals_begin_ray_and_trace(harness, worlds, world, direction):
    n = 4000
    first_hits, from_hook, from_next, second_hits, special, stray = _run(harness, worlds[world], n, direction)
    assert special == 0 and stray == 0
    # the run does exercise what it is about: most first hits go on inside the end-of-walk phase, and both outcomes of the
    # second ray occur
    assert first_hits == from_hook + from_next and from_hook > n // 10
    assert 0 < second_hits < first_hits


def test_a_start_outside_the_grid_is_left_to_the_ray_finished_phase(harness, worlds):
    """The sparse world has voxels in its outermost layers: with the light going up and out, some hit points step out of the
    grid, and the hook must leave those lanes alone."""
    first_hits, from_hook, from_next, _, _, _ = _run(harness, worlds["sparse"], 4000, (INV, INV, INV))
    assert from_next > 0 and from_hook > 0


@pytest.mark.parametrize("direction", [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.6, 1e-13, 0.8)])
def test_a_special_direction_takes_no_hook_path(harness, worlds, direction):
    """A direction with a component that is zero or below 2^-40 is `special` for every start: the hook declines every lane (as the
    render kernel switches the path off for such a light), and the pairs still equal the oracle."""
    first_hits, from_hook, from_next, _, special, _ = _run(harness, worlds["sparse"], 3000, direction)
    assert special == 1 and from_hook == 0 and from_next == first_hits > 0
