"""The walk every frame stage shares (csrc/vxrt_reproject.hpp: rp_launch_shape, rp_wave_pixel), restated once for the stages'
host harnesses (tests/tools/frame_launch.h), on the edge shapes of a frame: W in {1, 63, 64, 65} x H in {1, 3, 4, 5}, 65535 x 1
and 1 x 65535, each on 1 and on 256 compute units, with and without a summary.  tests/tools/frame_launch_check.cpp asserts that
every pixel is visited exactly once by the lanes inside the frame (tests/tools/frame_launch.h) and the launch shape: grid == tiles without a
summary, 1 <= grid <= 2 * cus with one.  No GPU."""
import os
import subprocess

from tests import helpers


def test_every_pixel_once_on_the_edge_shapes(tmp_path):
    tools = os.path.join(helpers.ROOT, "tests", "tools")
    exe = str(tmp_path / "frame_launch_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(tools, "hoststub"), "-o", exe,
                           os.path.join(tools, "frame_launch_check.cpp"), "-w"])
    out = helpers.run_harness(exe)
    assert int(out.split()[0]) == 18 * 2 * 2, out  # every frame on both device sizes, with and without a summary
