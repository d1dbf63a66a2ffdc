"""CPU checks of the temporal filter (include/vxrt.h, vxrt_reproject_frame): the two restatements of tests/ref_reproject.py
against each other on random frames with small camera moves, hand-derived cases with an axis-aligned ortho camera whose
window makes one pixel one voxel and dyadic colours (the arithmetic is exact), the limits, the kernel's per-pixel code
(csrc/vxrt_reproject.hpp) compiled for the host (tests/tools/reproject_check.cpp) against the restatement -- records,
colours, BGRA8 and summary bit-equal, every index checked -- and one quality test on the CPU oracle: along a moving camera
path a one-sample frame is closer to its converged counterpart with the reprojected history than without."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import ref_denoise as R
from tests import ref_reproject as T
from tests.helpers import build_harness, run_harness_files
from tests.test_denoise_host import LIMITS

F32 = np.float32
FLOOR = 0x84000005   # the face y = 5 seen from above (axis 1, not toward)
OTHER = 0x84000006
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _case(W, H, ortho):
    return T.random_case(W, H, ortho)


@functools.lru_cache(maxsize=None)
def _want(W, H, ortho, history=True):
    rec, summary = T.run_case(_case(W, H, ortho), history=history)
    rec.setflags(write=False)
    return rec, summary


# ---- the restatements against each other -------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", T.FRAMES)
@pytest.mark.parametrize("ortho", (False, True))
def test_the_restatements_agree(W, H, ortho):
    case = _case(W, H, ortho)
    for history in (True, False):
        a, sa = _want(W, H, ortho, history)
        b, sb = T.run_case(case, scalar=True, history=history)
        assert np.array_equal(R.bits(a), R.bits(b)), (W, H, ortho, history)
        assert sa == sb and sa[0] == sa[1] + sa[2] + sa[3] == int((case["keys"] != 0).sum())
        assert history or sa[1] == 0
    print("reproject random case", W, H, ortho, "hit, reused, offscreen, rejected", _want(W, H, ortho)[1])


def test_the_random_cases_reach_every_outcome():
    """over the frames that are more than a few pixels: every outcome occurs, a history at max_history stays there, and no
    NaN from behind a foreign key reaches a finite pixel's output"""
    for ortho in (False, True):
        case = _case(130, 70, ortho)
        rec, (hit, reused, offscreen, rejected) = _want(130, 70, ortho)
        assert reused > hit // 4 and rejected > 0 and (offscreen > 0 or ortho)
        assert rec[..., 3].max() == case["max_history"] and set(np.unique(rec[..., 3])) >= {0.0, 1.0, 2.0}
        assert (case["keys_prev"] == T.FOREIGN).sum() > 100 and np.isnan(case["hist"]).any()
        finite_in = np.isfinite(case["color"]).all(-1)
        assert np.isfinite(rec[finite_in]).all()


# ---- hand-derived cases ------------------------------------------------------------------------------------------------
# An ortho camera looking down -y with right = +x and up = +z over a W x H = 8 x 4 frame and the window (2, 2): the ray of
# pixel (x, y) starts at pos + ((x / 4 - 1) * 2 * 2, 0, (y / 2 - 1) * 2) = pos + (x - 4, 0, y - 2): one pixel is one voxel,
# and with pos = (4, 10, 2) pixel (x, y) looks down onto (x, 5, y) of the floor face FLOOR.
HW, HH = 8, 4
WINDOW = (2.0, 2.0)
DOWN, UPZ, RIGHTX = (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)


def _cam(dx=0.0, dz=0.0):
    return ((4.0 + dx, 10.0, 2.0 + dz), DOWN, UPZ, RIGHTX)


def _both(color, keys, cur, prev, hist, keys_prev, max_history=32, ortho=True):
    kw = dict(max_history=max_history, ortho=ortho, ortho_size=WINDOW)
    a, sa = T.reproject(color, keys, cur, prev, hist, keys_prev, **kw)
    b, sb = T.reproject(color, keys, cur, prev, hist, keys_prev, scalar=True, **kw)
    assert np.array_equal(R.bits(a), R.bits(b)) and sa == sb
    return a, sa


def _floor(value=0.5):
    color = np.zeros((HH, HW, 3), F32)
    color[..., 0] = value
    color[..., 1] = np.arange(HW) / 8.0
    return color, np.full((HH, HW), FLOOR, np.uint32)


def _history(n=3.0):
    hist = np.zeros((HH, HW, 4), F32)
    hist[..., 0] = 0.25 * np.arange(HW) + np.arange(HH)[:, None] * 4.0
    hist[..., 2] = 0.125
    hist[..., 3] = n
    return hist


def test_identity_camera():
    """fx = x, fy = y exactly: one tap of weight 1, m = the history, n' = n + 1, out = m + (c - m) / n'"""
    color, keys = _floor()
    hist = _history(3.0)
    rec, summary = _both(color, keys, _cam(), _cam(), hist, keys)
    assert summary == (32, 32, 0, 0) and (rec[..., 3] == 4.0).all()
    want = hist[..., :3] + (color - hist[..., :3]) / F32(4)
    assert np.array_equal(rec[..., :3], want)
    assert rec[1, 2, 0] == 4.5 + (0.5 - 4.5) / 4 and rec[1, 2, 2] == 0.125 - 0.125 / 4


def test_a_shift_by_whole_pixels():
    """the camera moved by +2 voxels along x since the previous frame: pixel x shows what pixel x + 2 showed; the columns 6
    and 7 look at points the previous frame had at fx = 8 = W (no tap in the frame) and 9 (beyond): offscreen, {c, 1}"""
    color, keys = _floor()
    hist = _history(1.0)
    rec, summary = _both(color, keys, _cam(2.0), _cam(), hist, keys)
    assert summary == (32, 24, 8, 0)
    assert np.array_equal(rec[:, :6, :3], hist[:, 2:, :3] + (color[:, :6] - hist[:, 2:, :3]) / F32(2)) and (rec[:, :6, 3] == 2.0).all()
    assert np.array_equal(rec[:, 6:, :3], color[:, 6:]) and (rec[:, 6:, 3] == 1.0).all()
    # and along y by -1: row y shows what row y - 1 showed; row 0 has fy = -1: its lower taps are row 0 with weight 0 -- in the
    # frame, not accepted: rejected
    rec, summary = _both(color, keys, _cam(0.0, -1.0), _cam(), hist, keys)
    assert summary == (32, 24, 0, 8)
    assert np.array_equal(rec[1:, :, :3], hist[:-1, :, :3] + (color[1:] - hist[:-1, :, :3]) / F32(2))
    assert np.array_equal(rec[0, :, :3], color[0]) and (rec[0, :, 3] == 1.0).all()


def test_a_half_pixel_shift_is_the_two_pixel_average():
    """fx = x + 1/2: the taps x and x + 1 at weight 1/2 each, sw = 1, m their average; column 7 has its right tap outside
    the frame: m = (h / 2) / (1 / 2) = h.  nmin is the smaller n of the two"""
    color, keys = _floor()
    hist = _history(2.0)
    hist[:, 3, 3] = 6.0
    rec, summary = _both(color, keys, _cam(0.5), _cam(), hist, keys)
    assert summary == (32, 32, 0, 0)
    m = (hist[:, :-1, :3] + hist[:, 1:, :3]) * F32(0.5)
    assert np.array_equal(rec[:, :7, :3], m + (color[:, :7] - m) / F32(3)) and (rec[:, :7, 3] == 3.0).all()
    assert np.array_equal(rec[:, 7, :3], hist[:, 7, :3] + (color[:, 7] - hist[:, 7, :3]) / F32(3))
    assert rec[2, 0, 0] == F32(8.125) + F32(0.5 - 8.125) / F32(3)


def test_foreign_taps_renormalise_and_reject():
    """quarter-pixel shifts in x and y: weights 9/16, 3/16, 3/16, 1/16.  One tap of a foreign key (NaN behind it) drops out
    and the rest renormalise; a tap with n = 0 likewise; all taps foreign: rejected"""
    color, keys = _floor()
    hist = _history(1.0)
    prev_keys = keys.copy()
    prev_keys[1, 3] = OTHER              # the (x0 + 1, y0) tap of pixel (2, 1)
    hist[1, 3, :3] = NAN
    hist[2, 6, 3] = 0.0                  # the (x0 + 1, y0 + 1) tap of pixel (5, 1)
    prev_keys[0:2, 0:2] = OTHER          # every tap of pixel (0, 0)
    rec, summary = _both(color, keys, _cam(0.25, 0.25), _cam(), hist, prev_keys)
    assert np.isfinite(rec[keys != 0][:, :3]).all()
    w = [F32(0.5625), F32(0.1875), F32(0.1875), F32(0.0625)]
    h = hist[..., 0]
    sw = (w[0] + w[2]) + w[3]
    m = ((w[0] * h[1, 2] + w[2] * h[2, 2]) + w[3] * h[2, 3]) / sw
    assert rec[1, 2, 0] == m + (F32(0.5) - m) / F32(2) and rec[1, 2, 3] == 2.0
    sw = (w[0] + w[1]) + w[2]
    m = ((w[0] * h[1, 5] + w[1] * h[1, 6]) + w[2] * h[2, 5]) / sw
    assert rec[1, 5, 0] == m + (F32(0.5) - m) / F32(2)
    assert np.array_equal(rec[0, 0], (*color[0, 0], 1.0))
    assert summary[3] >= 1 and summary[0] == 32 == sum(summary[1:])
    # every previous key foreign: every pixel with a tap in the frame is rejected
    rec, summary = _both(color, keys, _cam(0.25, 0.25), _cam(), hist, np.full_like(keys, OTHER))
    assert summary == (32, 0, 0, 32) and np.array_equal(rec[..., :3], color) and (rec[..., 3] == 1.0).all()


def test_the_previous_camera_facing_away_is_offscreen():
    color, keys = _floor()
    hist = _history(1.0)
    cur = ((4.0, 10.0, 2.0), DOWN, UPZ, RIGHTX)
    prev = ((4.0, 10.0, 2.0), (0.0, 1.0, 0.0), UPZ, RIGHTX)
    rec, summary = _both(color, keys, cur, prev, hist, keys, ortho=False)
    assert summary[0] == summary[2] > 0 and summary[1] == summary[3] == 0
    assert np.array_equal(rec[..., :3], color) and np.array_equal(rec[..., 3] == 1.0, keys != 0)
    # facing the same way: the identity, every hit pixel reused
    rec, summary = _both(color, keys, cur, cur, hist, keys, ortho=False)
    assert summary[1] > 0 and summary[2] == 0


def test_a_constant_sequence_counts_up_to_max_history_and_stays():
    color, keys = _floor(0.75)
    hist = None
    for frame in range(7):
        rec, summary = _both(color, keys, _cam(), _cam(), hist, keys if hist is not None else None, max_history=4)
        assert (rec[..., 3] == min(frame + 1, 4)).all() and np.array_equal(rec[..., :3], color)
        assert summary == ((32, 0, 0, 32) if frame == 0 else (32, 32, 0, 0))
        hist = rec


def test_a_miss_pixel_is_copied_and_is_never_a_source():
    color, keys = _floor()
    keys = keys.copy()
    keys[1, 4] = 0
    color[1, 4] = (9.0, -3.0, NAN)
    first, summary = _both(color, keys, _cam(), _cam(), None, None)
    assert summary == (31, 0, 0, 31)
    assert np.array_equal(R.bits(first[1, 4]), R.bits(np.array([9.0, -3.0, NAN, 0.0], F32)))
    # next frame the pixel is a hit: its own history is the miss record (key 0, n = 0): rejected; with a half-pixel shift
    # its left neighbour (3, 1) averages pixels 3 and 4 of the history and takes pixel 3 alone
    color2, keys2 = _floor()
    rec, summary = _both(color2, keys2, _cam(), _cam(), first, keys)
    assert summary == (32, 31, 0, 1) and np.array_equal(rec[1, 4], (*color2[1, 4], 1.0))
    rec, summary = _both(color2, keys2, _cam(0.5), _cam(), first, keys)
    assert np.array_equal(rec[1, 3, :3], first[1, 3, :3] + (color2[1, 3] - first[1, 3, :3]) / F32(2))
    assert np.isfinite(rec[..., :3]).all()


def test_either_history_pointer_null_gives_every_hit_pixel_a_new_mean():
    color, keys = _floor()
    keys = keys.copy()
    keys[0, 0] = 0
    for hist, prev_keys in ((None, None), (_history(), None), (None, keys)):
        rec, summary = _both(color, keys, _cam(0.25), _cam(), hist, prev_keys)
        assert np.array_equal(rec[..., :3], color) and np.array_equal(rec[..., 3], (keys != 0).astype(F32))
        assert summary[0] == 31 and summary[1] == 0


# ---- the kernel's code on the host -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "reproject_check")


def _run(exe, tmp_path, case, history=True, fb=True, cout=True, alias=False, summary=True, cus=256):
    H, W = case["keys"].shape
    n = W * H
    ortho = case["ortho"]
    o, d = R.primary_rays(W, H, *case["cur"], ortho=ortho, ortho_size=case["ortho_size"])
    flags = int(ortho) | 2 * history | 4 * fb | 8 * cout | 16 * alias | 32 * summary
    arrays = [np.array(T.camera_constants(W, H, 90.0, case["ortho_size"]), F32), np.concatenate(case["prev"]).astype(F32), case["color"],
              case["keys"], o, d]
    if history:
        arrays += [case["hist"], case["keys_prev"]]
    raw, stdout = run_harness_files(exe, tmp_path, [0, W, H, flags, case["max_history"], cus, 0, 0], *arrays)
    out = {"rec": raw[:16 * n].view(F32).reshape(H, W, 4)}
    at = 16 * n
    if cout:
        out["color"], at = raw[at:at + 12 * n].view(F32).reshape(H, W, 3), at + 12 * n
    if fb:
        out["fb"], at = raw[at:at + 4 * n].reshape(H, W, 4), at + 4 * n
    if summary:
        out["summary"], at = tuple(int(v) for v in raw[at:at + 16].view(np.uint32)), at + 16
    assert at == raw.size and int(stdout.split()[0]) >= 3 * n
    return out


def _assert_equal(got, want, what):
    rec, summary = want
    assert np.array_equal(R.bits(got["rec"]), R.bits(rec)), what
    if "color" in got:
        assert np.array_equal(R.bits(got["color"]), R.bits(rec[..., :3])), what
    if "fb" in got:
        assert np.array_equal(got["fb"], R.bgra8(rec[..., :3])), what
    if "summary" in got:
        assert got["summary"] == summary, what


@pytest.mark.parametrize("W,H", T.FRAMES)
@pytest.mark.parametrize("ortho", (False, True))
def test_the_kernel_code_on_the_host_equals_the_restatement(harness, tmp_path, W, H, ortho):
    case = _case(W, H, ortho)
    _assert_equal(_run(harness, tmp_path, case), _want(W, H, ortho), (W, H, ortho))
    _assert_equal(_run(harness, tmp_path, case, alias=True, cus=1), _want(W, H, ortho), (W, H, ortho, "alias"))  # waves on many tiles
    _assert_equal(_run(harness, tmp_path, case, fb=False, cout=False, summary=False), _want(W, H, ortho), (W, H, ortho, "bare"))
    _assert_equal(_run(harness, tmp_path, case, history=False), _want(W, H, ortho, False), (W, H, ortho, "no history"))


def test_the_harness_under_sanitizers(tmp_path):
    """the harness's own main, stand-alone, under ASan and UBSan"""
    exe = str(tmp_path / "reproject_check_san")
    root = helpers.ROOT
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(root, "tests", "tools", "hoststub"), "-o", exe,
                        os.path.join(root, "tests", "tools", "reproject_check.cpp"), "-w"], capture_output=True, text=True)
    if r.returncode != 0 and any(s in r.stderr.lower() for s in ("sanitize", "asan", "ubsan")):
        pytest.skip("no sanitizer runtime for the host compiler")
    assert r.returncode == 0, r.stderr[-2000:]
    for ortho in (False, True):
        _assert_equal(_run(exe, tmp_path, _case(65, 33, ortho)), _want(65, 33, ortho), ortho)
        _assert_equal(_run(exe, tmp_path, _case(65, 5, ortho), history=False, alias=True), _want(65, 5, ortho, False), ortho)


# ---- the limits ----------------------------------------------------------------------------------------------------------
def test_limits(harness, tmp_path):
    for W, H, ok in LIMITS:
        for m, mok in ((0, False), (1, True), (65535, True), (65536, False)):
            assert R.frame_ok(W, H) == ok and T.history_ok(m) == mok
            raw, _ = run_harness_files(harness, tmp_path, [2, np.uint32(W).astype(np.int32), np.uint32(H).astype(np.int32), 0, m, 0, 0, 0])
            assert raw.view(np.uint32).tolist() == [int(ok), int(mok)], (W, H, m)


# ---- quality on the CPU oracle -----------------------------------------------------------------------------------------
PATH_POSES = 16


def camera_path(dims, vxo):
    """16 poses from camera A: a step forward-right and a slight turn per frame"""
    (px, py, pz), _, _, _ = helpers.camera("A", dims, vxo)
    euler = helpers.CAMERAS["A"][1]
    out = []
    for j in range(PATH_POSES):
        f, u, r = vxo.get_directions((euler[0], euler[1] + 0.01 * j, euler[2]))
        out.append(((px + 0.35 * j, py - 0.05 * j, pz + 0.25 * j), f, u, r))
    return out


def test_the_history_brings_a_one_sample_frame_closer_to_the_converged_one(vxo):
    """terrain, 96 x 64, one occlusion sample on every hit pixel, 16 poses of a camera that translates and turns a little per
    frame (frame number j at pose j), max_history 16: the last frame's output against the mean over 64 frame numbers at the
    last pose (the oracle's accumulation), mean squared error over hit pixels before and after.  On the last frame more than
    half of the hit pixels are reused and both other outcomes occur.  Measured: 2429 hit pixels, 1708 reused, 10 offscreen,
    711 rejected; ratio after / before 0.549 (profiles/reproject.md; the spatial filter alone reaches 0.758 on this frame)."""
    W, H = 96, 64
    w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32)
    path = camera_path(w.dims, vxo)
    kw = dict(shadow=1, bounce_samples=1, bounce_all_hits=1)
    hist = keys_prev = None
    for j, cam in enumerate(path):
        noisy = w.render(vxo.make_params(W, H, *cam, frame_number=j, **kw), fb=np.zeros((H, W, 4), np.uint8), want_color=True,
                         want_hit=True)
        o, d = R.primary_rays(W, H, *cam)
        keys = R.keys_np(noisy["hit"], w.dims, o, d)
        rec, summary = T.reproject(noisy["color"], keys, cam, path[max(j - 1, 0)], hist, keys_prev, max_history=16)
        hist, keys_prev = rec, keys
    acc = np.zeros((H, W, 4), F32)
    for frame in range(1, 65):
        conv = w.render(vxo.make_params(W, H, *path[-1], frame_number=frame, **kw), fb=np.zeros((H, W, 4), np.uint8),
                        want_color=True, accum=acc, accum_reset=frame == 1)
    hit = keys != 0
    assert np.array_equal(hit, noisy["hit"] >= 0) and (acc[..., 3][hit] == 64).all() and 0.2 < hit.mean() < 0.8
    n_hit, reused, offscreen, rejected = summary
    print("reproject quality: last frame hit %d reused %d offscreen %d rejected %d, mean n %.2f" % (*summary, rec[..., 3][hit].mean()))
    assert n_hit == hit.sum() and reused > n_hit // 2 and rejected > 0 and offscreen > 0
    assert np.array_equal(R.bits(rec[~hit][:, :3]), R.bits(noisy["color"][~hit]))

    def mse(a):
        return float(((a.astype(np.float64) - conv["color"])[hit] ** 2).mean())

    before, after = mse(noisy["color"]), mse(rec[..., :3])
    print("reproject quality: mse before %.6g after %.6g ratio %.4f" % (before, after, after / before))
    assert before > 0 and after < before
