"""The read limit cases (tests/read_limit_cases.py) without a GPU: the launch caps read from the sources, every case past the
cap it targets, a copy of the sources with any one cap raised 64-fold leaving some case short (so raising a cap fails here
instead of quietly emptying tests/test_gpu_read_limits.py), read_region's launch arithmetic restated and held to the
figures worked out by hand, its mapping of workgroups and lanes to words storing every word of a box exactly once, the
identities of the large cases held against the restatements (oracle/ref_region.py, tests/ref_surface.py,
tests/ref_denoise.py) at small sizes, and the boxes and frames that the host harnesses can run in seconds through the
kernels' own code with every index checked (tests/tools/region_check.cpp, tests/tools/denoise_check.cpp)."""
import os
import re

import numpy as np
import pytest

from tests import read_limit_cases as F
from tests import ref_denoise as RD
from tests import ref_surface as RS
from tests.helpers import build_harness, run_harness
from tests.test_denoise_host import _run as _denoise_harness

F32 = np.float32


def _short(caps):
    return [(case.name, what, value, bound) for case in F.LAUNCH_CASES for what, value, bound in case.reach(caps)
            if not value > bound]


# ---- the caps --------------------------------------------------------------------------------------------------------------
def test_caps_are_read_from_the_sources():
    c = F.read_caps()
    assert all(v > 0 for v in c.values())
    assert (c["dn_max_side"], c["dn_max_pixels"], c["dn_max_iterations"]) == (RD.MAX_SIDE, RD.MAX_PIXELS, RD.MAX_ITERATIONS)
    assert all(RD.frame_ok(*f) for f in F.THIN_FRAMES) and all(RD.frame_ok(*f) for f, _ in F.LIMIT_FRAMES)
    assert F.surf_rows(F.SHARE_DIMS) == 4718592 and F.surf_share(F.SHARE_DIMS, c) == (18432, 72)
    assert F.dn_grid(65535, 5, True, c) == (1024, 1) and F.dn_grid(5, 65535, False, c) == (1, 16384)


def test_the_launch_restatement_gives_the_figures_worked_out_by_hand():
    c = F.read_caps()
    a = F.read_launch(F.ALONG_Z_DIMS, c)
    assert (a.wpr, a.L, a.nxc, a.rpw, a.nyg, a.zsteps) == (1, 1, 1, 64, 1, 8)
    assert (a.blocks, a.gx, a.gy, a.surplus) == ((1 << 21) + 5, 1 << 20, 3, (1 << 20) - 5)
    assert F.region_words(F.ALONG_Z_DIMS) * 4 == (256 << 20) + 640
    b = F.read_launch(F.ALONG_ROWS_DIMS, c)
    assert (b.wpr, b.L, b.nxc, b.rpw, b.nyg, b.zsteps, b.pad_mask) == (1 << 26, 64, 1 << 20, 1, 2, 8, 0x7FFFFFFF)
    assert (b.blocks, b.gx, b.gy, b.surplus) == (1 << 21, 1 << 20, 2, 0)
    assert F.region_words(F.ALONG_ROWS_DIMS) * 4 == 512 << 20
    o, d = F.ALONG_ROWS_ORIGIN, F.ALONG_ROWS_DIMS
    assert o[0] + d[0] - 1 == 64 + 2 and o[0] + d[0] <= F.INT32_MAX and o[0] - 1 + d[0] - 1 < 64 + 2  # the most negative such start
    assert F.ladder_zsteps(c) == [1, 2, 4, 8]
    e = F.read_launch((32, 4096, 500), c)
    assert e.nxc * e.nyg == 64 and 64 * 16 < c["zsteps_blocks"] <= 64 * 32 and e.zsteps == 4
    m = [F.read_launch(d, c) for _, d in F.MAPPING_BOXES]
    assert tuple(x.wpr for x in m) == F.MAPPING_WPR
    assert [x.L for x in m] == [8, 16, 32, 64, 64, 64, 64] and [x.nxc for x in m] == [1, 1, 1, 1, 1, 2, 3]
    assert all(d[0] % 32 for _, d in F.MAPPING_BOXES) and all(d[1] % x.rpw for (_, d), x in zip(F.MAPPING_BOXES, m) if x.rpw > 1)


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


# ---- region reads ----------------------------------------------------------------------------------------------------------
def _stores_once(dims, caps):
    idx, (xw, yl, zl) = F.read_stores(dims, caps)
    n = F.region_words(dims)
    assert idx.size == n and np.array_equal(np.sort(idx), np.arange(n)), dims
    return xw, yl, zl


@pytest.mark.parametrize("k", range(len(F.LADDER_BOXES)))
def test_the_ladder_boxes_store_every_word_once(k):
    _stores_once(F.LADDER_BOXES[k][1], F.read_caps())


def test_the_mapping_boxes_store_every_word_once():
    caps = F.read_caps()
    for _, d in F.MAPPING_BOXES:
        xw, yl, zl = _stores_once(d, caps)
        assert xw.max() == F.read_launch(d, caps).wpr - 1 and yl.max() == d[1] - 1 and zl.max() == d[2] - 1


def test_twins_of_the_grid_y_boxes_store_every_word_once():
    """the two boxes of 2^21 workgroups scaled down, with grid_2d's first axis (and the workgroups that zsteps asks for) scaled
    down as far: three and two grid rows, surplus workgroups in the first"""
    caps = dict(F.read_caps(), grid_2d_x=1 << 6, zsteps_blocks=1 << 6)
    d = (1, 1, (1 << 12) + 160)
    a = F.read_launch(d, caps)
    assert (a.blocks, a.gx, a.gy, a.surplus) == ((1 << 7) + 5, 1 << 6, 3, (1 << 6) - 5)
    _stores_once(d, caps)
    d = ((1 << 17) - 1, 2, 1)
    b = F.read_launch(d, caps)
    assert (b.wpr, b.nxc, b.blocks, b.gy) == (1 << 12, 1 << 6, 1 << 7, 2)
    _stores_once(d, caps)


def test_the_tail_of_the_long_rows():
    """the world's rows arrive in the last three words of the 2^26, shifted by 28 bits, the last word cut to 31 bits; and at a
    small size a read equals the tail of the read that starts whole words before it"""
    from oracle import ref_region
    world = F.small_world()
    tail = F.along_rows_tail(world)
    o = F.ALONG_ROWS_ORIGIN
    assert (-o[0]) >> 5 == (1 << 26) - 3 and (-o[0]) & 31 == 28
    assert not tail[:, 0].any() and tail[:, 1:].any(1).all() and not (tail[:, 3] >> 31).any()
    for r in range(2):
        bits = np.unpackbits(tail[r].view(np.uint8), bitorder="little")
        assert np.array_equal(bits[32 + 28:32 + 28 + 64].astype(bool), world[:, o[1] + r, o[2]]) and bits.sum() == world[:, o[1] + r, o[2]].sum()
    for skip in (32, 96):
        d = (1000, 3, 2)
        whole = F.pack_region(ref_region.read_region(world, (-950, 9, 19), d)).reshape(6, -1)
        part = F.pack_region(ref_region.read_region(world, (-950 + skip, 9, 19), (d[0] - skip, 3, 2))).reshape(6, -1)
        assert np.array_equal(whole[:, skip // 32:], part) and part.any()
    import voxelengine_amd as vx
    v = np.random.default_rng(1).random((70, 3, 4)) < 0.5
    assert np.array_equal(F.pack_region(v), vx.pack_region(v))


def test_the_column_of_the_long_box():
    world = F.small_world()
    nz = F.along_z_nonzero(world)
    x, y, z = F.ALONG_Z_ORIGIN
    assert 10 < len(nz) < 64 and nz.min() >= -z and nz.max() < -z + 64 and 0 <= x < 64 and 0 <= y < 64


@pytest.fixture(scope="module")
def region_check(tmp_path_factory):
    return build_harness(tmp_path_factory, "region_check", "vxo_region.c")


def test_the_boxes_through_the_row_code_on_the_host(region_check):
    """region_row_word on the ladder and the mapping boxes, clipped as k_read_region clips, against the oracle on random
    worlds of the cases' sizes"""
    for (o, d), world in [(b, (8, 64, 64, 64)) for b in F.LADDER_BOXES] + [(b, (8, 8192, 64, 64)) for b in F.MAPPING_BOXES]:
        out = run_harness(region_check, "box", *world, *o, *d)
        assert int(out.split(" voxels set")[0].split()[-1]) > 0 and "failures 0" in out


# ---- surfaces ----------------------------------------------------------------------------------------------------------------
def _same_surface(a, b):
    return (np.array_equal(a.quads, b.quads) and np.array_equal(a.vertices, b.vertices) and np.array_equal(a.triangles, b.triangles)
            and np.array_equal(a.summary, b.summary))


def test_a_world_strictly_inside_its_box_gives_the_translated_surface():
    """a 12^3 world in a 40 x 50 x 60 box, in the far and in the near corner: CAP equals OPEN equals the OPEN surface of the
    world's own box grown by one voxel, moved"""
    world = np.random.default_rng(7).random((12, 12, 12)) < 0.5
    dims = (40, 50, 60)
    own = RS.extract(world, (-1, -1, -1), (14, 14, 14), RS.OPEN)
    assert len(own.quads) > 500
    for origin in (tuple(13 - d for d in dims), (-1, -1, -1)):
        want = F.translated(own, tuple(-1 - o for o in origin))
        for mode in (RS.CAP, RS.OPEN):
            assert _same_surface(RS.extract(world, origin, dims, mode), want), (origin, mode)
    assert not _same_surface(own, F.translated(own, (27, 37, 47)))
    assert F.SHARE_ORIGINS[0] == (65 - 256, 65 - 1024, 65 - 1024) and F.share_offset(F.SHARE_ORIGINS[0]) == (190, 958, 958)
    assert F.share_offset(F.SHARE_ORIGINS[1]) == (0, 0, 0)


def test_the_checkerboard_counts_and_its_first_records():
    dims = (32, 10, 6)
    world = F.checker(dims)
    for mode in (RS.CAP, RS.OPEN):
        s = RS.extract(world, (0, 0, 0), dims, mode)
        got = tuple(int(v) for v in s.summary)
        assert (got[0], got[1], got[2], 0, got[4:10], got[10:16]) == F.checker_summary(dims), mode
        assert np.array_equal(s.quads, RS.extract_scan(world, (0, 0, 0), dims, mode).quads)
    thin = RS.extract(world, (0, 0, 0), (1, dims[1], 3), RS.CAP)
    n = int(thin.summary[10])
    assert n == dims[1] * 3 // 2 and (thin.quads[:n, 1] >> 20 == 0).all()
    assert np.array_equal(s.quads[:n], thin.quads[:n]) and np.array_equal(s.vertices[:4 * n], thin.vertices[:4 * n])
    assert np.array_equal(s.triangles[:2 * n], thin.triangles[:2 * n])
    assert F.checker_summary(F.CHECKER_WORLD[:3]) == (1 << 27, 6 << 27, 6 << 27, 0, (1 << 27,) * 6, (1 << 27,) * 6)
    assert F.CHECKER_THIN[1] * F.CHECKER_THIN[2] // 2 == max(F.CHECKER_CAPACITIES)
    rows = F.checker_stamp_rows(dims)
    assert np.array_equal(np.repeat(rows.reshape(-1), dims[0] // 32), F.pack_region(world))
    assert not np.array_equal(F.checker(dims, 0), world)


# ---- the denoiser --------------------------------------------------------------------------------------------------------------
def _special_colours(c, rng):
    c = c.copy()
    H, W, _ = c.shape
    for v in F.SPECIALS:
        for _ in range(4):
            c[rng.integers(0, H), rng.integers(0, W), rng.integers(0, 3)] = F32(v)
    return c


def test_a_frame_of_tiles_denoises_to_tiles_of_the_small_result():
    """3 x 4 tiles of 23 x 17 with NaN, infinities and denormals among the colours: a tap on another tile's key is skipped by a
    select, as a tap outside the frame is"""
    W, H, tx, ty = 23, 17, 3, 4
    c, keys = RD.random_frame(W, H)
    c = _special_colours(c, np.random.default_rng(3))
    assert F.tiles_share_no_key(keys, tx, ty)
    big_c, big_k = F.tiled_frame(c, tx, ty), F.tiled_keys(keys, tx, ty)
    assert big_c.shape == (H * ty, W * tx, 3) and np.array_equal(big_k != 0, np.tile(keys != 0, (ty, tx)))
    assert len(np.unique(big_k[big_k != 0])) == tx * ty * len(np.unique(keys[keys != 0]))
    for n in F.DN_ITERATIONS:
        for k in F.DN_SCALES:
            small = RD.denoise_np(c, keys, n, k)
            assert np.array_equal(RD.bits(RD.denoise_np(big_c, big_k, n, k)), RD.bits(F.tiled_frame(small, tx, ty))), (n, k)
    # and it is the keys that keep the tiles apart
    assert not np.array_equal(RD.bits(RD.denoise_np(big_c, np.tile(keys, (ty, tx)), 3, 0.0)), RD.bits(F.tiled_frame(RD.denoise_np(c, keys, 3, 0.0), tx, ty)))


def test_no_two_tiles_of_the_large_frames_share_a_key():
    for frame, tile in F.LIMIT_FRAMES:
        _, keys = RD.random_frame(*tile)
        tx, ty = frame[0] // tile[0], frame[1] // tile[1]
        assert (tx * tile[0], ty * tile[1]) == frame and tx * ty < 1 << 18
        assert F.tiles_share_no_key(keys, tx, ty), frame
    assert not F.tiles_share_no_key(np.array([[0x80000005, 0x80000305]], np.uint32), 2, 1)  # 5 ^ 1 << 8 == 0x305 ^ 2 << 8


@pytest.fixture(scope="module")
def denoise_check(tmp_path_factory):
    return build_harness(tmp_path_factory, "denoise_check")


@pytest.mark.parametrize("W,H", F.THIN_FRAMES)
def test_the_thin_frames_through_the_kernel_code_on_the_host(denoise_check, tmp_path, W, H):
    c, keys = RD.random_frame(W, H)
    for n in F.DN_ITERATIONS:
        for k in F.DN_SCALES:
            want = F.denoised(W, H, k, n)
            staged = (n + (k > 0)) % 2
            col, px, stdout = _denoise_harness(denoise_check, tmp_path, c, keys, n, k, staged, True, n == 3)
            assert np.array_equal(RD.bits(col), RD.bits(want)), (W, H, n, k)
            assert np.array_equal(px, RD.bgra8(want)), (W, H, n, k)
    assert not np.array_equal(RD.bits(F.denoised(W, H, 0.0, 6)), RD.bits(F.denoised(W, H, 0.0, 3)))


@pytest.mark.parametrize("staged", (0, 1))
def test_special_values_through_the_kernel_code_on_the_host(denoise_check, tmp_path, staged):
    c, keys, mask = F.special_frame()
    assert (mask & (keys != 0)).sum() > 100 and (mask & (keys == 0)).sum() > 20
    for n in F.DN_ITERATIONS:
        for k in F.SPECIAL_SCALES:
            want = RD.denoise_np(c, keys, n, k)
            col, px, _ = _denoise_harness(denoise_check, tmp_path, c, keys, n, k, staged, True, False)
            assert np.array_equal(RD.bits(col), RD.bits(want)), (n, k)
            assert np.array_equal(px, RD.bgra8(want)), (n, k)
    assert np.isnan(want).any() and np.isinf(want).any()


def test_the_special_values_catch_an_addition_of_zero(denoise_check, tmp_path):
    """dn_filter skips a tap by a select; in a scratch copy of the header the tap is added with weight 0 instead, which
    lets a NaN or an infinity behind another key in: the special frame tells the two apart, the random frames of
    tests/ref_denoise.py (finite colours) do not"""
    import shutil
    import subprocess
    for sub in ("tests/tools", "voxelengine_amd/csrc", "include"):
        shutil.copytree(os.path.join(F.ROOT, sub), tmp_path / sub, ignore=shutil.ignore_patterns("*.so", "*.o", "*.hip", "__pycache__"))
    header = tmp_path / "voxelengine_amd" / "csrc" / "vxrt_denoise.hpp"
    text, old = header.read_text(), "sr = use ? sr + w * q.r : sr;"
    assert text.count(old) == 1
    header.write_text(text.replace(old, "sr = sr + (use ? 1.0f : 0.0f) * (w * q.r);"))
    exe = str(tmp_path / "denoise_check_changed")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + str(tmp_path / "tests" / "tools" / "hoststub"), "-o", exe,
                           str(tmp_path / "tests" / "tools" / "denoise_check.cpp"), "-w"])
    run = tmp_path / "run"
    run.mkdir()
    c, keys, _ = F.special_frame()
    col, _, _ = _denoise_harness(exe, run, c, keys, 1, 0.0, 0, False, False)
    assert not np.array_equal(RD.bits(col), RD.bits(RD.denoise_np(c, keys, 1, 0.0)))
    col, _, _ = _denoise_harness(denoise_check, run, c, keys, 1, 0.0, 0, False, False)
    assert np.array_equal(RD.bits(col), RD.bits(RD.denoise_np(c, keys, 1, 0.0)))
    c, keys = RD.random_frame(*F.SPECIAL_FRAME)
    col, _, _ = _denoise_harness(exe, run, c, keys, 1, 0.0, 0, False, False)
    assert np.array_equal(RD.bits(col), RD.bits(RD.denoise_np(c, keys, 1, 0.0)))


def test_the_keys_of_the_large_world_through_the_kernel_code_on_the_host(denoise_check, tmp_path):
    from tests.helpers import run_harness_files
    W, H = F.GUIDE_FRAMES[0]
    dims = F.GUIDE_WORLD[:3]
    hit = F.guide_hits(W, H)
    rng = np.random.default_rng(2)
    o = ((rng.random((H, W, 3)) * 3 - 1) * np.array(dims)).astype(F32)
    d = rng.normal(size=(H, W, 3)).astype(F32)
    raw, _ = run_harness_files(denoise_check, tmp_path, [1, W, H, dims[0], dims[1], dims[2], 0, 0], hit.astype(np.int64), o, d)
    want = RD.keys_np(hit, dims, o, d)
    assert np.array_equal(raw.view(np.uint32).reshape(H, W), want)
    assert np.array_equal(want, RD.keys_scalar(hit, dims, o, d))
    total = dims[0] * dims[1] * dims[2]
    assert np.array_equal(want != 0, (hit >= 0) & (hit < total)) and ((hit >= 1 << 32) & (hit < total)).sum() > 1000
    flat = want.reshape(-1)
    assert [bool(flat[i]) for i in range(len(F.GUIDE_HITS))] == [0 <= h < total for h in F.GUIDE_HITS]
