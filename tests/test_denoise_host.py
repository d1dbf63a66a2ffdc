"""CPU checks of the frame denoiser (include/vxrt.h, vxrt_frame_guides / vxrt_denoise_frame): the two restatements of
tests/ref_denoise.py against each other on random frames and rays, hand-derived cases with dyadic colours (the arithmetic
is exact), the key rule case by case, the workspace formula and the limits, the kernels' per-pixel code
(csrc/vxrt_denoise.hpp) compiled for the host (tests/tools/denoise_check.cpp) against the restatement -- colours and BGRA8
bit-equal in both instantiations, every index checked -- and one quality test on the CPU oracle: a one-sample frame is
closer to its converged counterpart after the filter than before."""
import functools
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import ref_denoise as R
from tests.helpers import build_harness, run_harness_files

F32 = np.float32
K5, KX, KY = 0x80000005, 0x84000005, 0x8A000007  # three distinct keys (faces x = 5 from above, y = 5, z = 7 from below)


@functools.lru_cache(maxsize=None)
def _frame(W, H):
    c, k = R.random_frame(W, H)
    c.setflags(write=False)
    k.setflags(write=False)
    return c, k


@functools.lru_cache(maxsize=None)
def _want(W, H, iterations, k):
    c, keys = _frame(W, H)
    out = R.denoise_np(c, keys, iterations, k)
    out.setflags(write=False)
    return out


# ---- the restatements against each other -------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", R.FRAMES)
@pytest.mark.parametrize("k", R.SCALES)
def test_the_filter_restatements_agree(W, H, k):
    """iterations 1 .. 6 as the chain of their steps (steps 16 and 32 exceed every frame here): after each step the numpy
    and the scalar form hold the same bits, so every iteration count agrees"""
    c, keys = _frame(W, H)
    a = b = c
    for i in range(6):
        a, b = R.iterate_np(a, keys, 1 << i, k), R.iterate_scalar(b, keys, 1 << i, k)
        assert np.array_equal(R.bits(a), R.bits(b)), (W, H, k, i)
        assert np.array_equal(R.bits(a), R.bits(_want(W, H, i + 1, k)))
    assert not np.array_equal(R.bits(a), R.bits(c)) or W * H == 1


def test_the_key_restatements_agree():
    rng = np.random.default_rng(5)
    dims = (48, 40, 56)
    H, W = 40, 50
    hit = rng.integers(-1, dims[0] * dims[1] * dims[2] + 3, (H, W))
    o = ((rng.random((H, W, 3)) * 3 - 1) * np.array(dims)).astype(F32)
    d = rng.normal(size=(H, W, 3)).astype(F32)
    d[rng.random((H, W, 3)) < 0.15] = 0          # zero components, whole zero directions among them
    o[::3] = np.floor(o[::3])                    # origins on planes: exact ties between axes
    d[::3] = np.sign(d[::3])
    a, b = R.keys_np(hit, dims, o, d), R.keys_scalar(hit, dims, o, d)
    assert np.array_equal(a, b)
    assert (a == 0).sum() == ((hit < 0) | (hit >= 48 * 40 * 56)).sum() > 0
    assert set(np.unique((a[a != 0] >> 26) & 31).tolist()) == {0, 1, 2}


# ---- hand-derived filter cases ---------------------------------------------------------------------------------------
def _both(c, keys, n, k):
    a, b = R.denoise_np(c, keys, n, k), R.denoise_scalar(c, keys, n, k)
    assert np.array_equal(R.bits(a), R.bits(b))
    return a


@pytest.mark.parametrize("n", (1, 3, 6))
@pytest.mark.parametrize("k", (0.0, 0.5))
def test_two_abutting_planes_do_not_bleed(n, k):
    """left half one face in one colour, right half another: every tap a pixel accepts has the pixel's own colour, the
    weights cancel in sc / sw (w * c / w with dyadic c: exact), and the output is the input"""
    c = np.zeros((9, 12, 3), F32)
    keys = np.full((9, 12), K5, np.uint32)
    c[:, :6] = (0.5, 0.25, 1.0)
    c[:, 6:] = (0.125, 2.0, 0.75)
    keys[:, 6:] = KX
    assert np.array_equal(_both(c, keys, n, k), c)


def test_a_miss_pixel_and_its_neighbours():
    """a miss (key 0) is copied whatever its colour; its neighbours skip it: row of five pixels of one face around a miss"""
    c = np.zeros((1, 5, 3), F32)
    c[0, :, 0] = (1.0, 2.0, 64.0, 4.0, 8.0)
    keys = np.array([[K5, K5, 0, K5, K5]], np.uint32)
    out = _both(c, keys, 1, 0.0)
    assert out[0, 2, 0] == 64.0
    # pixel 1: taps dx = -1, 0, +2 (pixel 0, itself, pixel 3) with dy = 0: w = h * 3/8 for h = 1/4, 3/8, 1/16
    # sw = 3/32 + 9/64 + 3/128 = 33/128, sc = 3/32 * 1 + 9/64 * 2 + 3/128 * 4 = 60/128
    assert out[0, 1, 0] == F32(F32(0.46875) / F32(0.2578125))
    # pixel 0: itself, pixel 1 (dx = 1); pixel 2 is a miss: (9/64 * 1 + 3/32 * 2) / (9/64 + 3/32) = (21/64) / (15/64)
    assert out[0, 0, 0] == F32(F32(0.328125) / F32(0.234375))
    assert np.array_equal(out[..., 1:], c[..., 1:])


def test_a_one_pixel_surface():
    """a face one pixel wide accepts its centre tap only: (9/64 * c) / (9/64) = c, for every iteration count and scale"""
    c = np.full((5, 5, 3), 0.5, F32)
    keys = np.full((5, 5), K5, np.uint32)
    c[2, 2] = (3.0, 0.0, -7.0)
    keys[2, 2] = KY
    for n in (1, 4):
        for k in (0.0, 2.0):
            out = _both(c, keys, n, k)
            assert np.array_equal(out[2, 2], c[2, 2])
            assert np.array_equal(out[0, 0], c[0, 0])  # a constant face stays constant


def test_a_hand_computed_neighbourhood_with_three_keys():
    """5 x 5 pixels, the centre's face is the plus sign through the centre; the corners' blocks belong to two other faces.
    Row weights h = (1/16, 1/4, 3/8, 1/4, 1/16).  Accepted taps of the centre: the middle row and the middle column.
    With colour r = 16 * x + y (dyadic):
      sw = 3/8 * (1/16 + 1/4 + 3/8 + 1/4 + 1/16) + 3/8 * (1/16 + 1/4 + 1/4 + 1/16) = 3/8 * (1 + 5/8) = 39/64
      sc = sum over the row (y = 2): 3/8 * h[x] * (16 x + 2) = 3/8 * (16 * 2 + 2) = 51/4   (sum h x = 2, sum h = 1)
         + sum over the column without the centre (x = 2): 3/8 * h[y] * (32 + y), h = 1/16, 1/4, 1/4, 1/16:
           3/8 * (32 * 5/8 + (0 + 1/4 + 3/4 + 4/16)) = 3/8 * (20 + 5/4) = 255/32
      c' = (51/4 + 255/32) / (39/64) = (663/32) * (64/39) = 34: the plus sign is symmetric about the centre, whose r is 34"""
    y, x = np.mgrid[0:5, 0:5]
    c = np.zeros((5, 5, 3), F32)
    c[..., 0] = 16 * x + y
    keys = np.where((x == 2) | (y == 2), K5, np.where(x < 2, KX, KY)).astype(np.uint32)
    out = _both(c, keys, 1, 0.0)
    assert out[2, 2, 0] == 34.0 and out[2, 2, 1] == 0.0
    # corner block KX at (0, 0): taps (0,0), (1,0), (0,1), (1,1) and (0, 3), (1, 3) ... x < 2 and y != 2: rows 0, 1, 3, 4;
    # for pixel (x, y) = (0, 0): dy in {0, 1} (rows 0, 1; row 2 is the plus), dx in {0, 1}:
    #   w = 9/64, 3/32 (dx), 3/32 (dy), 1/16; r = 0, 16, 1, 17: sc = 3/2 + 3/32 + 17/16 = 85/32, sw = 25/64 -> 6.8
    assert out[0, 0, 0] == F32(F32(2.65625) / F32(0.390625))
    # the colour stop: k = 1/256 on the centre: e = r(q) - 34, the row taps have |e| = 32, 16, 0, 16, 32 -> d2 = 1024, 256, 0:
    # stop = max(1 - d2 / 256, 0) = 0, 0, 1: row taps at distance 1 and 2 vanish; the column taps have |e| = 2, 1, 1, 2:
    # stop = 1 - 4/256 = 63/64, 1 - 1/256 = 255/256
    out = _both(c, keys, 1, 1.0 / 256)
    w = [F32(0.375 * 0.0625) * F32(63 / 64), F32(0.375 * 0.25) * F32(255 / 256), F32(0.375 * 0.375), F32(0.375 * 0.25) * F32(255 / 256),
         F32(0.375 * 0.0625) * F32(63 / 64)]
    sw = sc = F32(0)
    for yy in range(5):   # the contract's order: dy outer; the row's other taps have weight 0 and r finite: they add +0
        sw = F32(sw + w[yy])
        sc = F32(sc + F32(w[yy] * F32(32 + yy)))
    assert out[2, 2, 0] == F32(sc / sw)


# ---- guide key cases -------------------------------------------------------------------------------------------------
DIMS = (64, 32, 16)


def _key(v, o, d, dims=DIMS):
    hit = v[0] + dims[0] * (v[1] + dims[1] * v[2])
    a = R.key_scalar(hit, dims, o, d)
    b = R.keys_np(np.array([[hit]]), dims, np.array([[o]], F32), np.array([[d]], F32))[0, 0]
    assert a == int(b)
    return a


def _k(axis, toward, plane):
    return 1 << 31 | axis << 26 | toward << 25 | plane


def test_key_cases():
    # a ray along +x enters voxel (10, 3, 4) through its x = 10 face; along -x through x = 11
    assert _key((10, 3, 4), (-5.0, 3.5, 4.5), (1.0, 0.0, 0.0)) == _k(0, 1, 10)
    assert _key((10, 3, 4), (70.0, 3.5, 4.5), (-1.0, 0.0, 0.0)) == _k(0, 0, 11)
    # d_k == 0 on two axes: they are -inf and never win, even from inside the slab
    assert _key((10, 3, 4), (10.5, 40.0, 4.5), (0.0, -1.0, 0.0)) == _k(1, 0, 4)
    # an exact tie between x and y (t = 2 on both) resolves to the lower axis; y against z the same
    assert _key((2, 2, 0), (0.0, 0.0, 0.5), (1.0, 1.0, 0.0)) == _k(0, 1, 2)
    assert _key((0, 2, 2), (0.5, 0.0, 0.0), (0.0, 1.0, 1.0)) == _k(1, 1, 2)
    # the largest t wins: from (0, 0, 0) towards (1, 2, 4) / 8 the z face of voxel (1, 2, 4) is entered last... t = 8, 8, 8: x
    assert _key((1, 2, 4), (0.0, 0.0, 0.0), (0.125, 0.25, 0.5)) == _k(0, 1, 1)
    assert _key((1, 2, 5), (0.0, 0.0, 0.0), (0.125, 0.25, 0.5)) == _k(2, 1, 5)  # t = 8, 8, 10
    # the zero direction: every t is -inf, axis 0, not toward, plane v + 1 (defined, never produced by a render)
    assert _key((7, 0, 0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)) == _k(0, 0, 8)
    # the last voxel of the world; index -1; indices out of range
    assert _key((63, 31, 15), (100.0, 31.5, 15.5), (-1.0, 0.0, 0.0)) == _k(0, 0, 64)
    o, d = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    for hit in (-1, -2, 64 * 32 * 16, 64 * 32 * 16 + 5, 2 ** 40, -2 ** 62):
        assert R.key_scalar(hit, DIMS, o, d) == 0
        assert R.keys_np(np.array([[hit]]), DIMS, np.array([[o]], F32), np.array([[d]], F32))[0, 0] == 0


def test_keys_of_the_ortho_camera():
    """ortho rays share fwd and differ in origin: looking down -y onto a flat floor at y = 7 every pixel enters through the
    +y face plane 8, whatever its origin; a perspective pixel looking down sees the same face"""
    W, H = 8, 6
    pos, fwd, up, right = (16.0, 30.0, 8.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    o, d = R.primary_rays(W, H, pos, fwd, up, right, ortho=True, ortho_size=(4.0, 3.0))
    assert np.array_equal(d, np.broadcast_to(np.array(fwd, F32), d.shape)) and len(np.unique(o[..., 0])) == W
    vx, vz = np.floor(o[..., 0]).astype(np.int64), np.floor(o[..., 2]).astype(np.int64)
    hit = vx + 64 * (7 + 32 * vz)
    keys = R.keys_np(hit, DIMS, o, d)
    assert (keys == _k(1, 0, 8)).all() and np.array_equal(keys, R.keys_scalar(hit, DIMS, o, d))
    o, d = R.primary_rays(W, H, pos, fwd, up, right)
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=-1), 1, atol=1e-6)
    t = (8.0 - o[..., 1]) / d[..., 1]
    px, pz = o[..., 0] + t * d[..., 0], o[..., 2] + t * d[..., 2]
    inside = (px > 0.01) & (px < 63.99) & (pz > 0.01) & (pz < 15.99)
    hit = np.where(inside, np.floor(px).astype(np.int64) + 64 * (7 + 32 * np.floor(pz).astype(np.int64)), -1)
    keys = R.keys_np(hit, DIMS, o, d)
    assert inside.any() and (keys[inside] == _k(1, 0, 8)).all() and (keys[~inside] == 0).all()


# ---- the workspace formula and the limits ------------------------------------------------------------------------------
LIMITS = [(1, 1, True), (0, 5, False), (5, 0, False), (65535, 1, True), (1, 65535, True), (65536, 1, False), (1, 65536, False),
          (8192, 8192, True), (8193, 8192, False), (65535, 1024, True), (65535, 1025, False), (1920, 1080, True), (2 ** 31, 1, False)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "denoise_check")


def test_workspace_formula_and_limits(harness, tmp_path):
    for W, H, ok in LIMITS:
        assert R.frame_ok(W, H) == ok
        assert R.workspace_bytes(W, H) == (2 * W * H * 16 if ok else 0)
        raw, _ = run_harness_files(harness, tmp_path, [2, np.uint32(W).astype(np.int32), np.uint32(H).astype(np.int32), 0, 0, 0, 0, 0])
        assert raw[:8].view(np.uint32).tolist() == [int(ok), 0] and int(raw[8:16].view(np.uint64)[0]) == R.workspace_bytes(W, H), (W, H)
    assert R.workspace_bytes(8192, 8192) == 1 << 31


# ---- the kernels' code on the host -------------------------------------------------------------------------------------
def _run(harness, tmp_path, c, keys, n, k, staged, fb, alias):
    H, W = keys.shape
    kb = int(np.array([k], F32).view(np.int32)[0])
    raw, stdout = run_harness_files(harness, tmp_path, [0, W, H, n, int(staged), int(fb), int(alias), kb], c, keys)
    col = raw[:12 * W * H].view(F32).reshape(H, W, 3)
    px = raw[12 * W * H:].reshape(H, W, 4) if fb else None
    assert raw.size == (16 if fb else 12) * W * H
    return col, px, stdout


@pytest.mark.parametrize("W,H", R.FRAMES)
@pytest.mark.parametrize("staged", (0, 1))
def test_the_kernel_code_on_the_host_equals_the_restatement(harness, tmp_path, W, H, staged):
    c, keys = _frame(W, H)
    for n in R.ITERATIONS:
        for k in R.SCALES:
            alias = (n + staged + (k > 0)) % 2
            col, px, stdout = _run(harness, tmp_path, c, keys, n, k, staged, True, alias)
            want = _want(W, H, n, k)
            assert np.array_equal(R.bits(col), R.bits(want)), (W, H, staged, n, k)
            assert np.array_equal(px, R.bgra8(want)), (W, H, staged, n, k)
            assert int(stdout.split()[0]) >= W * H
    # without a framebuffer; a single iteration whose output aliases its input (the pack runs on its own)
    col, px, _ = _run(harness, tmp_path, c, keys, 1, 0.75, staged, False, True)
    assert px is None and np.array_equal(R.bits(col), R.bits(_want(W, H, 1, 0.75)))


def test_the_key_code_on_the_host_equals_the_restatement(harness, tmp_path):
    rng = np.random.default_rng(9)
    for dims in ((48, 40, 56), (1 << 24, 3, 5), (2, 1 << 24, 1 << 14)):
        total = dims[0] * dims[1] * dims[2]
        H, W = 30, 41
        hit = rng.integers(0, total, (H, W))
        hit[rng.random((H, W)) < 0.1] = -1
        hit[0, :6] = (total, total + 1, total - 1, 0, -5, 2 ** 62)
        o = ((rng.random((H, W, 3)) * 3 - 1) * np.array(dims)).astype(F32)
        d = rng.normal(size=(H, W, 3)).astype(F32)
        d[rng.random((H, W, 3)) < 0.15] = 0
        o[::3] = np.floor(o[::3])
        d[::3] = np.sign(d[::3])
        raw, _ = run_harness_files(harness, tmp_path, [1, W, H, dims[0], dims[1], dims[2], 0, 0], hit.astype(np.int64), o, d)
        assert np.array_equal(raw.view(np.uint32).reshape(H, W), R.keys_np(hit, dims, o, d)), dims


def test_the_harness_under_sanitizers(tmp_path):
    """the harness's own main, stand-alone, under ASan and UBSan on a staged and a direct run"""
    import os
    exe = str(tmp_path / "denoise_check_san")
    root = helpers.ROOT
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(root, "tests", "tools", "hoststub"), "-o", exe,
                        os.path.join(root, "tests", "tools", "denoise_check.cpp"), "-w"], capture_output=True, text=True)
    if r.returncode != 0 and any(s in r.stderr.lower() for s in ("sanitize", "asan", "ubsan")):
        pytest.skip("no sanitizer runtime for the host compiler")
    assert r.returncode == 0, r.stderr[-2000:]
    c, keys = _frame(65, 33)
    for staged in (0, 1):
        col, px, _ = _run(exe, tmp_path, c, keys, 3, 0.75, staged, True, False)
        assert np.array_equal(R.bits(col), R.bits(_want(65, 33, 3, 0.75)))


# ---- quality on the CPU oracle -----------------------------------------------------------------------------------------
def test_the_filter_brings_a_one_sample_frame_closer_to_the_converged_one(vxo):
    """terrain, camera A, 96 x 64, one occlusion sample on every hit pixel: the frame of frame number 1 against the mean over
    frame numbers 1 .. 64 (the oracle's accumulation), mean squared error over hit pixels before and after 4 iterations
    without colour stop.  Measured ratio after / before: 0.66 (profiles/denoise.md)."""
    W, H = 96, 64
    w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32)
    pos, f, u, r = helpers.camera("A", w.dims, vxo)
    kw = dict(shadow=1, bounce_samples=1, bounce_all_hits=1)
    noisy = w.render(vxo.make_params(W, H, pos, f, u, r, frame_number=1, **kw), fb=np.zeros((H, W, 4), np.uint8), want_color=True,
                     want_hit=True)
    acc = np.zeros((H, W, 4), F32)
    for frame in range(1, 65):
        conv = w.render(vxo.make_params(W, H, pos, f, u, r, frame_number=frame, **kw), fb=np.zeros((H, W, 4), np.uint8),
                        want_color=True, accum=acc, accum_reset=frame == 1)
    hit = noisy["hit"] >= 0
    assert (acc[..., 3][hit] == 64).all() and 0.2 < hit.mean() < 0.8
    o, d = R.primary_rays(W, H, pos, f, u, r)
    keys = R.keys_np(noisy["hit"], w.dims, o, d)
    assert np.array_equal(keys != 0, hit) and len(np.unique(keys)) > 50
    out = R.denoise_np(noisy["color"], keys, 4, 0.0)
    assert np.array_equal(out[~hit], noisy["color"][~hit])

    def mse(a):
        return float(((a.astype(np.float64) - conv["color"])[hit] ** 2).mean())

    before, after = mse(noisy["color"]), mse(out)
    print("denoise quality: mse before %.6g after %.6g ratio %.4f" % (before, after, after / before))
    assert before > 0 and after < before
