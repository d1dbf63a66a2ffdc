"""The deferred coarse starts of the wave tracer (voxelengine_amd/csrc/vxrt_wave2.hpp: begin_ray_deferred,
phase_end_deferred, start_pending) compiled for the HOST and driven as a round of the persistent kernels drives them --
tight-box phase, end-of-walk phase, ray-finished phase, ONE start_pending for the walks both recorded, probes -- by one lane
that lives across all rays (tests/tools/host_defer_check.cpp).  For every ray of the adversarial families (zero, tiny and
denormal direction components, starts on far faces, origins outside the grid, rays that miss the world, wide grids) hit,
steps, position, normal, voxel and the three probe counters equal the oracle's, and no load leaves the tables' slack."""
import os
import re
import subprocess

import pytest

from tests import grid_shape_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    cc = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "tests", "tools", "hoststub"),
          "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(ROOT, "tests", "tools", "host_defer_check.cpp"),
          "-x", "c", os.path.join(ROOT, "oracle", "vxo_trace.c"), os.path.join(ROOT, "oracle", "vxo_world.c"),
          os.path.join(ROOT, "oracle", "vxo_render.c"), "-lm", "-lpthread", "-w"]
    subprocess.check_call(cc)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("hdc"), "host_defer_check")


@pytest.fixture(scope="module")
def harness_small_caps(tmp_path_factory):
    """The wide-grid field caps at 3 / 2 steps: a walk re-arms its packed counters (and CF_OFF_*) every few cells."""
    return _build(tmp_path_factory.mktemp("hdc_cap"), "host_defer_check_caps", ("-DVXRT_FIELD_CAP_XZ=3u", "-DVXRT_FIELD_CAP_Y=2u"))


def _run_out(exe, *args):
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "mismatches 0 of %d" % args[3] in out.stdout, out.stdout[-2000:]
    assert "outside it 0)" in out.stdout, out.stdout[-2000:]  # zero stray loads
    m = re.search(r"new rays (\d+), restarts (\d+), outside the grid (\d+); rounds with nothing pending (\d+)", out.stdout)
    return [int(v) for v in m.groups()], out.stdout


def _run(exe, *args):
    return _run_out(exe, *args)[0]


@pytest.mark.parametrize("factor,edge,density,n", [(8, 64, 0.01, 20000), (8, 64, 0.3, 10000), (16, 128, 0.002, 10000),
                                                   (32, 256, 0.0005, 6000)])
def test_deferred_starts_in_kernel_order_equal_oracle(harness, factor, edge, density, n):
    new_rays, restarts, outside, idle = _run(harness, factor, edge, density, n)
    # the run does exercise what it is about: every ray starts deferred, brick misses restart deferred, some starts land
    # outside the grid (the lane then meets the end-of-walk phase a round later), and most rounds have nothing pending
    assert new_rays == n and restarts > n // 20 and outside > n // 100 and idle > 0


@pytest.mark.parametrize("factor,sx,sy,sz,density,n", [(8, 32768, 64, 64, 0.000005, 20000), (8, 16384, 64, 128, 0.00002, 20000)])
def test_deferred_starts_on_wide_grids(harness, harness_small_caps, factor, sx, sy, sz, density, n):
    """Wide grids: start_walk also writes the CF_OFF_* words, from start_pending as from the phases before."""
    assert _run(harness, factor, sx, density, n, sy, sz)[0] == n
    assert _run(harness_small_caps, factor, sx, density, n, sy, sz)[0] == n


@pytest.mark.parametrize("factor,edge,density,n", [(8, 64, 0.01, 20000), (8, 64, 0.3, 10000)])
def test_deferred_starts_with_wide_grid_code_on_ordinary_grids(harness_small_caps, factor, edge, density, n):
    new_rays, restarts, outside, idle = _run(harness_small_caps, factor, edge, density, n, edge, edge, 1)
    assert new_rays == n and restarts > n // 20


@pytest.mark.parametrize("name", ["O1", "O2", "O3", "W2", "W3", "W5", "W6"])
def test_deferred_starts_on_grids_long_in_y_and_z(harness, harness_small_caps, name):
    """The shapes of tests/grid_shape_cases.py that a dense voxel array holds (f = 8), long walks along whichever axis is long
    included, with the product's caps and re-armed every 3 / 2 steps."""
    case = G.BY_NAME[name]
    assert case.factor == 8
    sx, sy, sz = case.dims
    for exe in (harness, harness_small_caps):
        counts, out = _run_out(exe, 8, sx, G.density(case), 20000, sy, sz)
        assert counts[0] == 20000 and "UNSUSPECTED EXITS" not in out, out[-2000:]
        long_walks = int(re.search(r"rays of more than 1024 steps (\d+)", out).group(1))
        exhausted = int(re.search(r"without a hit (\d+)", out).group(1))
        if max(case.cells) >= 1024:
            assert long_walks > 100, out
        if max(case.cells) >= 2048:
            assert exhausted > 100, out
