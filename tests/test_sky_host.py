"""CPU checks of the sky on frames (include/vxrt.h, vxrt_sky_frame): the two restatements of tests/ref_sky.py against each
other on the random cases of tests/sky_cases.py, whole frames and lists of pixels; what those cases exercise (checked on the
restatement alone, so that a case set cannot hide a branch); the hand-derived cases with the expected numbers written out;
the kernel's per-pixel code (csrc/vxrt_sky.hpp) compiled for the host (tests/tools/sky_check.cpp) against the restatement --
colours, BGRA8 and summary bit-equal, every index checked, at several task cuts --; the limits and the order of the refusals
(tests/tools/sky_args_check.cpp); the export and the Python mirror's structure."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import ref_denoise as R
from tests import ref_sky as SK
from tests import sky_cases as SC
from tests.helpers import build_harness, run_harness, run_harness_files

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _case(W, H, ortho, pose):
    return SC.random_case(W, H, ortho, pose)


@functools.lru_cache(maxsize=None)
def _want(W, H, ortho, pose, set_index=1):
    out = SC.run_case(_case(W, H, ortho, pose), SC.PARAM_SETS[set_index])
    out[0].setflags(write=False)
    return out


def _sets_of(W, H):
    """the parameter sets a frame runs under: all of them on the small frames, three on the larger ones"""
    return range(len(SC.PARAM_SETS)) if W * H <= 400 else (1, 6, 9)


# ---- the restatements against each other -------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,ortho,pose", SC.CASES)
def test_the_restatements_agree(W, H, ortho, pose):
    case = _case(W, H, ortho, pose)
    for s in _sets_of(W, H) if W * H <= 1200 else (1,):
        a = _want(W, H, ortho, pose, s)
        b = SC.run_case(case, SC.PARAM_SETS[s], scalar=True)
        what = (W, H, ortho, pose, s)
        assert np.array_equal(R.bits(a[0]), R.bits(b[0])), what
        assert a[1] == b[1], what
        for k in SK.COUNTERS:
            assert np.array_equal(a[2][k], b[2][k]), (what, k)
        for group in ("copied", "no_cloud"):
            for k, v in a[2][group].items():
                assert np.array_equal(v, b[2][group][k]), (what, group, k)
        miss, hit, ground, sun, cloud, fogged = a[1]
        assert miss + hit == W * H and ground + sun <= miss and cloud <= miss and fogged <= hit
        copied = sum(int(v.sum()) for v in a[2]["copied"].values())
        assert copied + fogged == hit
        keep = a[2]["hit"] & ~a[2]["fogged"]
        assert np.array_equal(R.bits(a[0].reshape(-1, 3)[keep]), R.bits(case["color"].reshape(-1, 3)[keep]))
    print("sky random case", W, H, ortho, pose, "miss, hit, ground, sun, cloud, fogged", _want(W, H, ortho, pose)[1])


def test_a_list_of_pixels_equals_the_whole_frame():
    W, H, ortho, pose = 130, 9, False, "up"
    whole = _want(W, H, ortho, pose)
    rng = np.random.default_rng(5)
    pixels = np.stack([rng.integers(0, W, 200), rng.integers(0, H, 200)], -1)
    for scalar in (False, True):
        part = SC.run_case(_case(W, H, ortho, pose), SC.PARAM_SETS[1], scalar=scalar, pixels=pixels)
        assert np.array_equal(R.bits(part[0]), R.bits(whole[0][pixels[:, 1], pixels[:, 0]]))
        assert part[1][0] + part[1][1] == 200


def test_the_random_cases_reach_every_branch():
    """on the restatement alone, over the case set: every counter, every reason a hit is copied and every reason a pixel has
    no cloud, the fog at fog_max and below it, NaN inputs on hits and misses, keys with an axis field above 2 -- and the
    clouds, the glow exponent and the octaves each change something"""
    seen = dict.fromkeys(SK.COUNTERS + tuple("copied_" + k for k in SK.COPIED) + tuple("no_cloud_" + k for k in SK.NO_CLOUD) +
                         ("at_fog_max", "below_fog_max", "nan_hit", "nan_miss", "axis_above_2", "partial_cloud"), 0)
    for W, H, ortho, pose in SC.CASES:
        case = _case(W, H, ortho, pose)
        out, summary, info = _want(W, H, ortho, pose)
        for k, v in zip(SK.COUNTERS, summary):
            seen[k] += v
        for k in SK.COPIED:
            seen["copied_" + k] += int(info["copied"][k].sum())
        for k in SK.NO_CLOUD:
            seen["no_cloud_" + k] += int(info["no_cloud"][k].sum())
        fog_max = F32(case["params"]["fog_max"])
        seen["at_fog_max"] += int((info["fogged"] & (info["f"] == fog_max)).sum())
        seen["below_fog_max"] += int((info["fogged"] & (info["f"] < fog_max)).sum())
        nan = np.isnan(case["color"]).any(-1).reshape(-1)
        seen["nan_hit"] += int((nan & info["hit"]).sum())
        seen["nan_miss"] += int((nan & info["miss"]).sum())
        assert not np.isnan(out.reshape(-1, 3)[info["miss"]]).any() or pose == "axis"
        seen["axis_above_2"] += int(((case["keys"].reshape(-1) >> 26) & 31 > 2).sum())
        seen["partial_cloud"] += int(((info["alpha"] > 0) & (info["alpha"] < 1)).sum())
        if W * H > 1000 and pose == "up":
            bits = [R.bits(_want(W, H, ortho, pose, s)[0]) for s in (1, 6, 9)]  # glow 1 and octaves 6; glow 6; no clouds
            assert not np.array_equal(bits[0], bits[1]) and not np.array_equal(bits[0], bits[2]) and not np.array_equal(bits[1], bits[2])
    # what the random poses do not give: a horizontal ray under the clouds (h == 0), a cloud plane too far away (t = 84 * 2^20), one
    # at an infinite t (a denormal h) and a noise cell beyond 2^30
    for d, p in (((1.0, 0.0, 0.0), {}), ((1.0, 2.0 ** -20, 0.0), {}), ((1.0, 1e-39, 0.0), {}), ((0.0, 1.0, 0.0), dict(cloud_scale=2.0 ** 28))):
        info = SC.run_case(SC.one_pixel((8.0, 16.0, 8.0), d, flags=SK.CLOUDS, **p))[2]
        for k in SK.NO_CLOUD:
            seen["no_cloud_" + k] += int(info["no_cloud"][k].sum())
    print("sky branches", seen)
    assert all(v > 0 for v in seen.values()), seen


# ---- hand-derived cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(SC.HAND_CASES)))
def test_hand_derived_cases(index):
    case, color, summary = SC.HAND_CASES[index]()
    for scalar in (False, True):
        got = SC.run_case(case, scalar=scalar)
        assert np.array_equal(R.bits(got[0][0, 0]), R.bits(np.asarray(color, F32))), (index, scalar, got[0])
        assert got[1] == summary, (index, scalar, got[1])


def test_an_ortho_frame_of_misses_has_one_colour():
    """d = (0.25, 0.5, 0.75) on every pixel: h = 0.5, a = 0.5, a4 = 0.0625; s = (0, 0, 1), sd = 0.75, g = 0.5625, k = 0.28125;
    e = smooth(clamp01((0.75 - 0.5) / 0.25)) = 1: the disc: sun_color on every pixel"""
    case = SC.ortho_frame()
    for scalar in (False, True):
        out, summary, _ = SC.run_case(case, scalar=scalar)
        assert (out == np.array([1.0, 0.5, 0.25], F32)).all() and summary == (64, 0, 0, 64, 0, 0)
    out, summary, _ = SC.run_case(case, dict(cos_inner=1.0, cos_outer=0.875))  # outside the disc: the gradient and the glow
    want = [F32(z) + (F32(0.75) - F32(z)) * F32(0.0625) + F32(s) * F32(0.28125) for z, s in zip((0.25, 0.5, 1.0), (1.0, 0.5, 0.25))]
    assert (out == np.array(want, F32)).all() and summary == (64, 0, 0, 0, 0, 0)
    # with clouds every pixel has its own point on the cloud plane: the colours differ
    out, summary, _ = SC.run_case(case, dict(flags=SK.CLOUDS, cos_inner=1.0, cos_outer=0.875, cloud_y=60.0, cloud_scale=1.0, cloud_cover=0.75))
    assert len(np.unique(R.bits(out).reshape(-1, 3), axis=0)) > 8 and summary[4] > 8


# ---- the kernel's code on the host -------------------------------------------------------------------------------------
FIELDS = [("struct_size", "<u4"), ("ortho", "<i4"), ("flags", "<u4"), ("glow_log2", "<u4"), ("octaves", "<u4"), ("seed", "<u4"),
          ("zenith", "<f4", 3), ("horizon", "<f4", 3), ("ground", "<f4", 3), ("sun_color", "<f4", 3), ("cloud_color", "<f4", 3), ("sun_dir", "<f4", 3),
          ("glow_strength", "<f4"), ("ground_fade", "<f4"), ("cos_inner", "<f4"), ("cos_outer", "<f4"), ("cloud_y", "<f4"), ("cloud_scale", "<f4"),
          ("cloud_offset", "<f4", 2), ("cloud_max_t", "<f4"), ("cloud_cover", "<f4"), ("cloud_sharp", "<f4"), ("cloud_fade", "<f4"),
          ("fog_start", "<f4"), ("fog_density", "<f4"), ("fog_max", "<f4"), ("cam", "<f4", 12), ("reserved_", "<i4")]


def _packed(case, p):
    """the 208 bytes of the call's vxrt_sky_params"""
    d = dict(SK.DAY, **dict(case["params"], **(p or {})))
    rec = np.zeros(1, np.dtype(FIELDS))
    assert rec.itemsize == 208
    for name in rec.dtype.names:
        if name in d:
            rec[name] = d[name]
    rec["struct_size"], rec["ortho"] = 208, int(case["ortho"])
    rec["cam"] = np.concatenate([np.asarray(v, F32) for v in case["cam"]])
    return rec


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "sky_check")


def _run(exe, tmp_path, case, p=None, fb=True, summary=True, alias=False, cus=256):
    H, W = case["keys"].shape
    n = W * H
    o, d = R.primary_rays(W, H, *case["cam"], ortho=case["ortho"], ortho_size=case["ortho_size"])
    io = int(fb) | 2 * summary | 4 * alias
    raw, stdout = run_harness_files(exe, tmp_path, [0, W, H, io, cus, 0, 0, 0], _packed(case, p), case["color"], case["keys"], o, d)
    out = {"color": raw[:12 * n].view(F32).reshape(H, W, 3)}
    at = 12 * n
    if fb:
        out["fb"], at = raw[at:at + 4 * n].reshape(H, W, 4), at + 4 * n
    if summary:
        out["summary"], at = tuple(int(v) for v in raw[at:at + 24].view(np.uint32)), at + 24
    assert at == raw.size and int(stdout.split()[0]) >= 2 * n  # (a key and a colour store per pixel at the least)
    return out


def _assert_equal(got, want, what):
    color, summary = want[:2]
    assert np.array_equal(R.bits(got["color"]), R.bits(color)), what
    if "fb" in got:
        assert np.array_equal(got["fb"], R.bgra8(color)), what
    if "summary" in got:
        assert got["summary"] == summary, what


@pytest.mark.parametrize("W,H,ortho,pose", SC.CASES)
def test_the_kernel_code_on_the_host_equals_the_restatement(harness, tmp_path, W, H, ortho, pose):
    """under every parameter set of the frame; the colour output aliasing the input with the counting launch of one compute
    unit (waves on many tiles), of three, and the plain launch without framebuffer and summary"""
    case = _case(W, H, ortho, pose)
    what = (W, H, ortho, pose)
    for s in _sets_of(W, H):
        _assert_equal(_run(harness, tmp_path, case, SC.PARAM_SETS[s]), _want(W, H, ortho, pose, s), (what, s))
    _assert_equal(_run(harness, tmp_path, case, SC.PARAM_SETS[1], alias=True, cus=1), _want(W, H, ortho, pose), (what, "alias"))
    _assert_equal(_run(harness, tmp_path, case, SC.PARAM_SETS[1], cus=3), _want(W, H, ortho, pose), (what, "three units"))
    _assert_equal(_run(harness, tmp_path, case, SC.PARAM_SETS[1], fb=False, summary=False), _want(W, H, ortho, pose), (what, "bare"))


def test_the_hand_derived_cases_through_the_harness(harness, tmp_path):
    for index, make in enumerate(SC.HAND_CASES):
        case, color, summary = make()
        got = _run(harness, tmp_path, case)
        assert np.array_equal(R.bits(got["color"][0, 0]), R.bits(np.asarray(color, F32))) and got["summary"] == summary, (index, got)
    case = SC.ortho_frame()
    _assert_equal(_run(harness, tmp_path, case, dict(flags=SK.CLOUDS, cloud_y=60.0, cloud_scale=1.0, cloud_cover=0.75)),
                  SC.run_case(case, dict(flags=SK.CLOUDS, cloud_y=60.0, cloud_scale=1.0, cloud_cover=0.75)), "ortho clouds")


def test_the_harness_under_sanitizers(tmp_path):
    """the harness's own main, stand-alone, under ASan and UBSan"""
    exe = str(tmp_path / "sky_check_san")
    tools = os.path.join(helpers.ROOT, "tests", "tools")
    san = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # whether the host compiler has the sanitizers' runtimes: a trivial program, built and run, so that nothing about the
    # harness itself can turn into a skip
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run(san + ["-o", str(tmp_path / "probe"), str(tmp_path / "probe.cpp")], capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime for the host compiler")
    r = subprocess.run(san + ["-I" + os.path.join(tools, "hoststub"), "-o", exe, os.path.join(tools, "sky_check.cpp"), "-lm", "-w"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for W, H, ortho, pose in ((67, 35, False, "level"), (130, 9, True, "up"), (64, 4, True, "axis")):
        _assert_equal(_run(exe, tmp_path, _case(W, H, ortho, pose), SC.PARAM_SETS[1]), _want(W, H, ortho, pose), (W, H, pose))
    _assert_equal(_run(exe, tmp_path, _case(65, 3, False, "high"), SC.PARAM_SETS[1], alias=True, cus=1), _want(65, 3, False, "high"), "alias")


# ---- the limits and the order of the refusals ----------------------------------------------------------------------------
def test_limits_and_refusal_order(tmp_path_factory):
    exe = build_harness(tmp_path_factory, "sky_args_check")
    out = run_harness(exe)
    assert int(out.split()[0]) == 216, out  # every CHECK of the program ran


# ---- the export and the Python mirror ----------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_the_mirror_matches_the_header():
    import voxelengine_amd as vx
    from voxelengine_amd import _native as N
    lib = vx.load()
    assert "vxrt_sky_frame" in vx.EXPORTS and hasattr(lib, "vxrt_sky_frame")
    assert C.sizeof(N.SkyParams) == 208 and vx.SKY_CLOUDS == 1
    assert [(name, C.sizeof(t)) for name, t in N.SkyParams._fields_] == [(f[0], 4 * (f[2] if len(f) > 2 else 1)) for f in FIELDS]
    sky = vx.Sky()
    day = dict(SK.DAY)
    assert {k: (tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in vars(sky).items()} == day
    p = vx.Sky(flags=vx.SKY_CLOUDS, sun_dir=(0.0, 3.0, 4.0), seed=9)._c(((1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)), True)
    assert (p.struct_size, p.ortho, p.flags, p.seed, p.reserved_) == (208, 1, 1, 9, 0) and list(p.sun_dir) == [0.0, 3.0, 4.0]
    assert list(p.cam.right) == [10.0, 11.0, 12.0] and p.fog_max == F32(day["fog_max"]) and list(p.cloud_offset) == [0.0, 0.0]
    assert vx.SkySummary(1, 2, 3, 4, 5, 6).fogged == 6
