"""The probed coarse set-up of the wave tracer (voxelengine_amd/csrc/vxrt_wave2.hpp: start_pending_probed) compiled for the
HOST and driven in the round order the render kernel builds on it -- end-of-walk phase (with a continuation hook),
ray-finished phase, set-up WITH its first probe, tight-box phase, probes -- by one lane that lives across all rays
(tests/tools/host_start_probe_check.cpp), on the two golden worlds.  Every ray, first rays and the second rays launched from
their hits by the hook or by the ray-finished phase, equals begin_ray + the undeferred phases on a fresh tracer and the C
oracle in hit, steps, position bits, normal, voxel and the three probe counters; after every set-up the lane's state equals,
field by field, that of the plain set-up followed by the first probe of a burst; no burst leaves `fix` behind; no load
leaves the tables' slack; and no advance leaves a grid unsuspected."""
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

INV = helpers.INV
N = 4000
FIELDS = ("hits", "walks", "occupied", "box_hit", "box_miss", "ended", "fix", "single", "outside", "special", "from_hook", "from_next",
          "brick_fix", "dir_special", "stray")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return helpers.build_harness(tmp_path_factory, "host_start_probe_check")


@pytest.fixture(scope="module")
def worlds(vxo, tmp_path_factory):
    """the golden worlds (tests/golden/make_golden.py) as files of dense voxel words, checked against the golden tables"""
    d = tmp_path_factory.mktemp("start_probe_worlds")
    out = {}
    dense = helpers.gen_dense(vxo, vxo.GEN_INT_TERRAIN, 128, 128, 128)
    out["terrain"] = ((128, 128, 128, 16), dense, make_golden.world_terrain())
    vox = np.random.default_rng(77).random((64, 64, 64)) < 0.02
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
    assert out.returncode == 0, out.stdout[-3000:]
    assert "mismatches 0 of %d" % n in out.stdout, out.stdout[-3000:]
    assert "UNSUSPECTED EXITS" not in out.stdout
    m = re.search(r"\(hits (\d+); walks set up (\d+): start cell occupied (\d+), tight box hit (\d+), missed (\d+); ended by the set-up's probe (\d+); "
                  r"fix (\d+), single-step (\d+), outside the grid (\d+), special (\d+); second rays by the hook (\d+), by the ray-finished phase (\d+); "
                  r"brick entries with fix (\d+); direction special (\d); loads outside the tables' slack (\d+)\)", out.stdout)
    assert m, out.stdout[-3000:]
    return dict(zip(FIELDS, (int(v) for v in m.groups())))


@pytest.mark.parametrize("world", ["terrain", "sparse"])
@pytest.mark.parametrize("direction", [(INV, INV, INV), (-0.3, 0.8, 0.52), (0.6, -0.2, -0.77)])
def test_rays_through_the_probed_set_up_equal_begin_ray_and_the_oracle(harness, worlds, world, direction):
    c = _run(harness, worlds[world], N, direction)
    assert c["stray"] == 0 and c["dir_special"] == 0
    # the run does exercise what it is about: more walks than rays (restarts after brick misses, second rays)
    assert c["walks"] > N and 0 < c["hits"] < N + c["from_hook"] + c["from_next"]
    # starts inside occupied cells -- the families built that way and most second rays -- with the tight box hit and missed in
    # the same round, and walks the set-up's own probe ends (single-step starts, starts on their exit face)
    assert c["occupied"] > N // 4 and c["box_hit"] > N // 8 and c["box_miss"] > 20
    if world == "sparse":  # (2 % of the voxels set: every coarse cell is occupied, so every start inside the grid is parked)
        assert c["occupied"] == c["walks"] - c["outside"] and c["ended"] == 0
    else:
        assert c["ended"] > 20
    # edge-rule starts, written behind the world entry by the harness: on one far face (fix, consumed by the set-up's probe)
    # and on several (single-step mode)
    assert c["fix"] > N // 50 and c["single"] > N // 50
    # starts outside the grid that miss the world, special rays, both ways to a second ray
    assert c["outside"] > N // 20 and c["special"] > N // 20 and c["from_hook"] > N // 10 and c["from_next"] > 0


def test_brick_entries_made_after_the_set_up_keep_their_fix_for_the_burst(harness, worlds):
    """A ray that enters a brick exactly on one of its far faces (the coarse walk crossed into the cell moving down that axis)
    starts its brick walk with fix != 0; the tight-box phase now runs after the set-up's probe has zeroed the lane's fix, and
    the burst's first probe must still consume the new one."""
    total = sum(_run(harness, worlds[w], N, (INV, INV, INV))["brick_fix"] for w in ("terrain", "sparse"))
    assert total > 0


@pytest.mark.parametrize("direction", [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.6, 1e-13, 0.8)])
def test_special_second_rays(harness, worlds, direction):
    """A fixed direction with a component that is zero or below 2^-40: the hook declines every lane, and every second ray is a
    `special` ray set up -- and probed once, in single-step mode -- by start_pending_probed."""
    c = _run(harness, worlds["sparse"], 3000, direction)
    assert c["dir_special"] == 1 and c["from_hook"] == 0 and c["from_next"] > 300 and c["special"] > c["from_next"]
