"""The wave tracer's fast per-ray set-up (voxelengine_amd/csrc/vxrt_wave2.hpp: WaveTracerT::begin_ray_inside_fast) compiled for
the HOST (tests/tools/host_bounce_hook_check.cpp).  The render kernel's end-of-walk hook launches a shadowed pixel's bounce
sample 0 with it, where no wave vote can fall back to the plain operators: the member either accepts a ray and leaves the lane
exactly as begin_ray_deferred would, or declines and touches nothing.  A few thousand random origins and directions in the two
golden worlds -- starts on faces, -0.0 and tiny components, directions far from unit length, starts outside the grid:
the member accepts exactly the rays of begin_ray_deferred's fast path from inside the grid; an accepted lane's registers and cold
fields equal begin_ray_deferred's bit for bit and its ray equals the C oracle's; a declined lane is unchanged."""
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


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return helpers.build_harness(tmp_path_factory, "host_bounce_hook_check")


@pytest.fixture(scope="module")
def worlds(vxo, tmp_path_factory):
    """the golden worlds (tests/golden/make_golden.py) as files of dense voxel words, checked against the golden tables"""
    d = tmp_path_factory.mktemp("bounce_hook_worlds")
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


@pytest.mark.parametrize("world", ["terrain", "sparse"])
def test_fast_set_up_equals_begin_ray_deferred_or_touches_nothing(harness, worlds, world):
    n = 6000
    out = subprocess.run([harness, worlds[world], str(n)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "mismatches 0 of %d" % n in out.stdout, out.stdout[-2000:]
    m = re.search(r"accepted (\d+), of them hits (\d+); declined (\d+): operand size (\d+), direction (\d+), start outside (\d+), "
                  r"start with a sign bit inside (\d+); loads outside the tables' slack (\d+)", out.stdout)
    accepted, hits, declined, by_size, by_dir, outside, negzero, stray = (int(v) for v in m.groups())
    assert accepted + declined == n and stray == 0
    # the run does exercise what it is about: most rays are accepted, both outcomes of an accepted ray occur, and every reason
    # to decline occurs
    assert accepted > n // 2 and 0 < hits < accepted
    assert min(by_size, by_dir, outside, negzero) > 20
