"""The map from a render launch to the frame and to the rows of the destination buffers, held on the CPU to the model of
tests/frame_shape_cases.py:
- the persistent kernel's pixel_coords (voxelengine_amd/csrc/vxrt_pixel_map.hpp) walked over the padded tile grid of every
  sharded case, mode, shard and buffer layout by tests/tools/pixel_map_check.cpp -- and the same walk over five changed
  copies of the header, each of which must fail (MUTATIONS names the cases that catch each);
- vxrt_compact_rows and sharding.ShardPlan.frame_row;
- the conditions the device tests rely on: the closed-form `written` mask is the oracle's, every row-owning shard sees hits
  and misses, the cap cases sit on their side of the caps read from the sources;
- the oracle against itself: per-strip renders (row_begin, row_end) reassemble to the full frame and their counters sum to
  it, which is what gives the device tests a per-shard reference for the counters.
k_render's own copy of the map (vxrt_kernels.hip) is tested on the device only: tests/test_gpu_frame_shapes.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import frame_shape_cases as FS
from tests import helpers

ROOT = helpers.ROOT
CSRC = os.path.join(ROOT, "voxelengine_amd", "csrc")
HEADER = os.path.join(CSRC, "vxrt_pixel_map.hpp")
LAYOUTS = (True, False)  # compact


def _build(tmp, header=None):
    exe = str(tmp / "pixel_map_check")
    cmd = ["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "tools", "hoststub"), "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "tools", "pixel_map_check.cpp"), "-w"]
    if header:
        cmd.append('-DPIXEL_MAP_HEADER="%s"' % header)
    subprocess.check_call(cmd)
    return exe


def _walk(exe, case, shard, compact, mode):
    cb, fn = FS.MODES[mode]
    out = helpers.run_harness(exe, case.W, case.H, case.strip_rows, case.strip_count, shard, int(compact), cb, fn)
    lines = out.splitlines()
    m = re.fullmatch(r"launch_rows (\d+) strip_shift (-?\d+)", lines[0])
    px = np.array([[int(v) for v in ln.split()] for ln in lines[1:-1]], np.int64).reshape(-1, 4)
    return int(m.group(1)), int(m.group(2)), px


def _violations(exe, case, shard, compact, mode):
    """the ways the harness's walk of one launch differs from the model (empty: it is the model's launch)"""
    cb, fn = FS.MODES[mode]
    launch_rows, shift, px = _walk(exe, case, shard, compact, mode)
    bad = []
    if launch_rows != case.launch_rows(shard, cb):
        bad.append("launch_rows")
    if shift != (case.strip_rows.bit_length() - 1 if case.strip_rows & (case.strip_rows - 1) == 0 else -1):
        bad.append("strip_shift")
    want = case.shard_mask(shard, mode)
    x, y, ty, out_row = px.T
    inside = (x >= 0) & (x < case.W) & (y >= 0) & (y < case.H)
    got = np.zeros_like(want, dtype=np.int64)
    np.add.at(got, (y[inside], x[inside]), 1)
    if not inside.all():
        bad.append("a pixel outside the frame")
    if (got > 1).any():
        bad.append("a pixel twice")
    if not np.array_equal(got > 0, want):
        bad.append("the set of pixels")
    x, y, ty, out_row = px[inside].T
    sharded = case.strip_count > 1
    if not np.array_equal(out_row, case.packed_row(y) if compact and sharded else y):
        bad.append("out_row")
    elif len(out_row) and out_row.max() >= case.buffer_rows(shard, compact) - FS.GUARD_ROWS:
        bad.append("out_row beyond the buffer")
    ref_ty = FS.thread_row(case.W, case.H, cb, fn)
    if not np.array_equal(ty, ref_ty[y, x]):
        bad.append("ty")
    return bad


def _launches(case):
    return [(s, c, m) for m in FS.MODES for s in range(case.strip_count) for c in LAYOUTS]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pixel_map"))


@pytest.mark.parametrize("case", FS.SHARDED + [FS.Case("29x27", 29, 27), FS.Case("16x64", 16, 64)], ids=lambda c: c.name)
def test_pixel_coords_is_the_models_launch(harness, case):
    for shard, compact, mode in _launches(case):
        assert _violations(harness, case, shard, compact, mode) == [], (case, shard, compact, mode)


def test_pixel_coords_on_the_tallest_sharded_frame(harness):
    for shard in range(2):
        for mode in ("plain", "checker_odd"):
            assert _violations(harness, FS.TALLEST_SHARDED, shard, True, mode) == [], (shard, mode)


# (what to replace, by what, the sharded cases whose walk then differs from the model)
MUTATIONS = {
    "the shift path used when strip_shift == -1": (
        "A.strip_shift >= 0 ? row >> A.strip_shift : row / sr", "row >> (A.strip_shift & 31)",
        {"61x92_12x4", "64x45_5x2"}),
    "/ strip_count dropped from the compact out_row of the checkerboard path": (
        "(uint32_t)A.strip_rows) / (uint32_t)A.strip_count) * (uint32_t)A.strip_rows +", "(uint32_t)A.strip_rows)) * (uint32_t)A.strip_rows +",
        {"72x93_8x3", "61x92_12x4", "40x30_16x5", "33x50_1x7", "64x45_5x2"}),
    "the ownership comparison off by one shard": (
        "!= (uint32_t)A.strip_index)", "!= ((uint32_t)A.strip_index + 1u) % (uint32_t)A.strip_count)",
        {"72x93_8x3", "61x92_12x4", "40x30_16x5", "33x50_1x7", "64x45_5x2"}),
    "the frame-parity term flipped": (
        "if (frame_number % 2 == 0)", "if (frame_number % 2 != 0)",
        {"72x93_8x3", "61x92_12x4", "40x30_16x5", "33x50_1x7", "64x45_5x2"}),
    "row < launch_rows turned into <=": (
        "c.live = row < A.launch_rows;", "c.live = row <= A.launch_rows;",
        {"72x93_8x3", "64x45_5x2"}),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_harness_catches_a_changed_map(tmp_path, name):
    """each change, applied to a scratch copy of the header, is caught, and by the cases that were chosen to reach it"""
    old, new, catchers = MUTATIONS[name]
    with open(HEADER) as f:
        text = f.read()
    assert text.count(old) == 1, (name, text.count(old))
    changed = tmp_path / "vxrt_pixel_map_changed.hpp"
    changed.write_text(text.replace(old, new))
    exe = _build(tmp_path, str(changed))
    caught = {c.name for c in FS.SHARDED if any(_violations(exe, c, *l) for l in _launches(c))}
    assert caught == catchers, (name, sorted(caught))


def test_compact_rows_and_shard_plan_are_the_models():
    import voxelengine_amd as vx
    from voxelengine_amd import sharding
    for case in FS.SHARDED + [FS.TALLEST_SHARDED] + FS.DEINTERLEAVE:
        total = 0
        for shard in range(case.strip_count):
            rows = case.rows_of(shard)
            total += len(rows)
            assert vx.compact_rows(case.H, case.strip_rows, case.strip_count, shard) == len(rows) == sum(
                e - b for b, e in case.strips_of(shard)), (case, shard)
            plan = sharding.ShardPlan(case.W, case.H, case.strip_rows, case.strip_count, shard)
            assert plan.local_rows == len(rows)
            assert [plan.frame_row(shard, k) for k in range(len(rows))] == rows.tolist(), (case, shard)
            assert np.array_equal(case.packed_row(rows), np.arange(len(rows)))  # packed in order, no gaps
            assert np.array_equal(np.concatenate([np.arange(b, e) for b, e in case.strips_of(shard)] + [np.zeros(0, int)]), rows)
        assert total == case.H
    assert vx.compact_rows(93, 8, 1, 0) == 93   # unsharded: the frame


def test_the_cases_reach_what_they_are_for():
    caps = FS.read_caps()
    cap = caps["max_scheduled_tile_rows"]
    assert FS.ceil_div(FS.TALL_ON.H, 8) == cap and FS.ceil_div(FS.TALL_OFF.H, 8) == cap + 1   # nty <= cap: a schedule; above: none
    assert FS.TALLEST.H == caps["max_height"] == FS.TALLEST_SHARDED.H and FS.TOO_TALL.H == caps["max_height"] + 1
    assert caps["max_height"] < 1 << 16 and caps["max_views"] == 16   # the packed row | view << 16 is exact up to here
    assert FS.TALLEST.H >> 1 == 32767
    assert FS.WIDE.W > 1 << 16
    for case in FS.DEINTERLEAVE:   # more 16-byte lanes than the capped grid has threads: the kernel's loop repeats
        assert case.W % 4 == 0 and case.W // 4 * case.H > caps["deinterleave_blocks"] * caps["deinterleave_threads"]
    by = FS.SHARDED_BY_NAME
    c = by["72x93_8x3"]
    assert c.strip_rows & (c.strip_rows - 1) == 0 and c.H % c.strip_rows == 5 and c.H % 2 == 1
    c = by["61x92_12x4"]
    assert c.strip_rows & (c.strip_rows - 1) != 0 and c.H % c.strip_rows == 8 and c.W % 8 != 0 and c.W % 2 == 1 and c.H % 2 == 0
    assert not FS.written(c.W, c.H, 1, 4)[:, 0::2].all(axis=0).any() and (2 * (c.H // 2 - 1) + 2 == c.H)  # ty = H/2 - 1 dies at y == H
    c = by["40x30_16x5"]
    assert [c.compact_rows(s) for s in range(5)] == [16, 14, 0, 0, 0]
    c = by["33x50_1x7"]
    assert c.strip_rows == 1
    c = by["64x45_5x2"]   # a launch row's two candidate frame rows 2 ty + 1, 2 ty + 2 (odd frame: 2 ty, 2 ty + 1) in different strips
    ty = np.arange(c.H >> 1)
    assert (c.owner(2 * ty + 1) != c.owner(2 * ty + 2)).any() and (c.owner(2 * ty) != c.owner(2 * ty + 1)).any()
    for c in FS.SHARDED:   # every case: more than one tile row in the checkerboard launches, and the shards partition the frame
        assert (c.H >> 1) > 8
        for mode in FS.MODES:
            masks = [c.shard_mask(s, mode) for s in range(c.strip_count)]
            assert np.array_equal(sum(m.astype(int) for m in masks), FS.written(c.W, c.H, *FS.MODES[mode]).astype(int))


@pytest.mark.parametrize("case", FS.SHARDED, ids=lambda c: c.name)
def test_written_mask_and_hit_mix_of_the_oracle(vxo, case):
    """A pixel is written iff two oracle renders over different stale backgrounds agree there: that set is the closed-form
    mask.  With camera A and the ray kinds of the sharded cases every row-owning shard has hits and misses among its written
    pixels (case 40x30: shard 0 only misses, shard 1 both) and every frame has bounce rays."""
    w = FS.world(vxo)
    for cam in ("A", "D"):
        for mode in FS.MODES:
            p = FS.params(vxo, case, cam, mode)
            a = w.render(p, fb=np.zeros((case.H, case.W, 4), np.uint8), nthreads=16)["fb"]
            b = w.render(p, fb=np.full((case.H, case.W, 4), 77, np.uint8), nthreads=16)["fb"]   # (alpha is 255 when written)
            assert np.array_equal((a == b).all(axis=2), FS.written(case.W, case.H, *FS.MODES[mode])), (cam, mode)
    for mode in FS.MODES:
        full = FS.oracle_full(vxo, case, "A", mode, **FS.HIT_MIX)
        assert full["stats"].bounce_rays > 0 and full["stats"].shadow_rays == full["stats"].primary_hits
        for shard in range(case.strip_count):
            m = case.shard_mask(shard, mode)
            hits = int((full["hit"][m] >= 0).sum())
            if case.name == "40x30_16x5":
                if mode == "plain":
                    assert (hits, int(m.sum())) == {0: (0, 640), 1: (390, 560)}.get(shard, (0, 0))
                assert (hits > 0) == (shard == 1)
            else:
                assert 0 < hits < int(m.sum()), (mode, shard)


@pytest.mark.parametrize("case", FS.SHARDED, ids=lambda c: c.name)
def test_oracle_strips_reassemble_and_their_counters_sum(vxo, case):
    w = FS.world(vxo)
    kw = FS.HIT_MIX
    for mode in FS.MODES:
        full = FS.oracle_full(vxo, case, "A", mode, **kw)
        fb = np.full((case.H, case.W, 4), 9, np.uint8)
        tot = dict.fromkeys(FS.RAY_COUNTERS + FS.PROBE_COUNTERS, 0)
        for shard in range(case.strip_count):
            st = FS.oracle_shard_stats(vxo, case, "A", mode, shard, **kw)
            assert st["primary_rays"] == int(case.shard_mask(shard, mode).sum()), (mode, shard)
            for k in tot:
                tot[k] += st[k]
            for b, e in case.strips_of(shard):
                w.render(FS.params(vxo, case, "A", mode, row_begin=b, row_end=e, **kw), fb=fb, nthreads=16)
        fs = full["stats"]
        assert tot == {**{k: int(getattr(fs, k)) for k in FS.RAY_COUNTERS}, **{k: int(getattr(fs.probes, k)) for k in FS.PROBE_COUNTERS}}
        wm = FS.written(case.W, case.H, *FS.MODES[mode])
        assert np.array_equal(fb[wm], full["fb"][wm]) and (fb[~wm] == 9).all(), mode
