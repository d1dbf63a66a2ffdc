"""Frame-shape cases of the render launches, and a model of the map from a launch to the frame and to the rows of the
destination buffers.  Shared by tests/test_frame_shapes_host.py (the persistent kernel's pixel_coords walked on the host,
vxrt_compact_rows, ShardPlan, the oracle against itself) and tests/test_gpu_frame_shapes.py (both render kernels and
k_deinterleave on the device).

The model restates include/vxrt.h and the reference's screenDispatch (Renderer.cu:183-196), not the kernels:
- a full launch is W x H threads, W x (H >> 1) under checkerboard; thread (tx, ty) owns pixel x = tx,
  y = ty, or under checkerboard y = 2 * ty + (x even) + (frame number even), and writes it when y < H;
- rows are cut into strips of `strip_rows`; strip s belongs to shard s % strip_count; a compact buffer holds the shard's
  strips packed in order, a full-size one holds them at their frame rows.

The caps live in voxelengine_amd/csrc; read_caps() reads them with regexes that must match exactly once."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = "voxelengine_amd/csrc/"

CAP_SOURCES = {  # name: (file, regex whose group 1 is the value); each must match exactly once
    "max_scheduled_tile_rows": (_CSRC + "vxrt_kernels.hpp", r"constexpr unsigned kMaxScheduledTileRows = (\d+);"),
    "max_height": (_CSRC + "vxrt_api.hip", r"if \(width == 0 \|\| height == 0 \|\| height > (\d+)u\)"),
    "deinterleave_blocks": (_CSRC + "vxrt_kernels.hip", r"if \(blocks > (\d+)\)\n\s+blocks = \1;"),
    "deinterleave_threads": (_CSRC + "vxrt_kernels.hip", r"hipLaunchKernelGGL\(k_deinterleave, dim3\(blocks, n_views\), dim3\((\d+)\)"),
    "max_views": (_CSRC + "vxrt_kernels.hpp", r"constexpr unsigned kMaxViews = (\d+);"),
}


def read_caps(root=ROOT):
    caps = {}
    for name, (path, rx) in CAP_SOURCES.items():
        with open(os.path.join(root, path)) as f:
            found = re.findall(rx, f.read())
        assert len(found) == 1, (name, path, rx, found)
        caps[name] = int(found[0])
    return caps


def ceil_div(a, b):
    return -(-a // b)


# ---- the model -----------------------------------------------------------------------------------------------------------
MODES = {"plain": (0, 3), "checker_even": (1, 4), "checker_odd": (1, 3)}  # name: (checkerboard, frame number)
GUARD_ROWS = 3


def written(W, H, checkerboard, frame_number):
    """(H, W) bool: the pixels a full launch writes"""
    if not checkerboard:
        return np.ones((H, W), bool)
    # y = 2 * ty + (x even) + (frame even) for some 0 <= ty < H >> 1
    d = np.arange(H, dtype=np.int64)[:, None] - (np.arange(W, dtype=np.int64)[None, :] % 2 == 0) - int(frame_number % 2 == 0)
    return (d >= 0) & (d % 2 == 0) & (d // 2 < H >> 1)


def thread_row(W, H, checkerboard, frame_number):
    """(H, W) int64: the row `ty` of the reference's thread that writes each pixel (it seeds the RNG and places the debug
    overlay), -1 where no thread writes"""
    y = np.repeat(np.arange(H, dtype=np.int64)[:, None], W, 1)
    if not checkerboard:
        return y
    x = np.arange(W, dtype=np.int64)[None, :]
    ty = (y - (x % 2 == 0) - (frame_number % 2 == 0)) // 2
    return np.where(written(W, H, checkerboard, frame_number), ty, -1)


class Case:
    """a frame of W x H pixels cut into strips of `strip_rows` rows for `strip_count` shards (1: unsharded)"""

    def __init__(self, name, W, H, strip_rows=16, strip_count=1, reaches=""):
        self.name, self.W, self.H, self.strip_rows, self.strip_count, self.reaches = name, W, H, strip_rows, strip_count, reaches

    def __repr__(self):
        return "Case(%s)" % self.name

    def owner(self, y):
        return (np.asarray(y) // self.strip_rows) % self.strip_count

    def packed_row(self, y):
        y = np.asarray(y)
        return (y // self.strip_rows // self.strip_count) * self.strip_rows + y % self.strip_rows

    def rows_of(self, shard):
        """the frame rows of `shard`, in the order of its compact buffer"""
        y = np.arange(self.H)
        return y[self.owner(y) == shard]

    def compact_rows(self, shard):
        return len(self.rows_of(shard))

    def strips_of(self, shard):
        """[(row_begin, row_end)] of the shard's strips"""
        n = ceil_div(self.H, self.strip_rows)
        return [(s * self.strip_rows, min((s + 1) * self.strip_rows, self.H)) for s in range(shard, n, self.strip_count)]

    def launch_rows(self, shard, checkerboard):
        """rows of the launch grid (include/vxrt.h: the reference's halved launch under checkerboard, else the shard's rows)"""
        if checkerboard:
            return self.H >> 1
        return self.compact_rows(shard) if self.strip_count > 1 else self.H

    def shard_mask(self, shard, mode):
        """(H, W) bool: the pixels the shard's launch writes"""
        cb, fn = MODES[mode]
        m = written(self.W, self.H, cb, fn)
        if self.strip_count > 1:
            m = m & (self.owner(np.arange(self.H)) == shard)[:, None]
        return m

    def buffer_rows(self, shard, compact):
        return (self.compact_rows(shard) if compact and self.strip_count > 1 else self.H) + GUARD_ROWS

    def expected_shard(self, full, stale, shard, compact, mode):
        """what the shard's buffer must hold after the launch.  `full`: the oracle's full-frame array (H, W, ...); `stale`: the
        buffer's contents before the launch, (buffer_rows, W, ...).  The stale pattern everywhere, guard rows included, except
        the oracle's values at the shard's written pixels, at row packed_row(y) of a compact buffer and at row y otherwise."""
        assert full.shape[:2] == (self.H, self.W) and stale.shape[:2] == (self.buffer_rows(shard, compact), self.W)
        out = stale.copy()
        ys, xs = np.nonzero(self.shard_mask(shard, mode))
        rows = self.packed_row(ys) if compact and self.strip_count > 1 else ys
        out[rows, xs] = full[ys, xs]
        return out

    def unpack(self, stale, shard, compact, into):
        """`into` (a full-frame array) with the shard's rows taken from its buffer `stale`: the background the oracle renders
        over to follow a buffer that is not cleared between frames"""
        rows = self.rows_of(shard) if self.strip_count > 1 else np.arange(self.H)
        into[rows] = stale[self.packed_row(rows) if compact and self.strip_count > 1 else rows]
        return into


SHARDED = [
    Case("72x93_8x3", 72, 93, 8, 3, "power-of-two strip height (strip_shift); last strip partial (5 rows); odd H"),
    Case("61x92_12x4", 61, 92, 12, 4, "division path; partial last strip of 8 rows; odd W with a ragged tile column; even H: "
                                      "checkerboard has the dead row y == H"),
    Case("40x30_16x5", 40, 30, 16, 5, "two strips for five shards: shards 2-4 own nothing"),
    Case("33x50_1x7", 33, 50, 1, 7, "one-row strips; strip_shift == 0"),
    Case("64x45_5x2", 64, 45, 5, 2, "odd strip height: under checkerboard, pairs straddle strips"),
]
SHARDED_BY_NAME = {c.name: c for c in SHARDED}
TALL_ON = Case("16x4096", 16, 4096, reaches="512 tile rows: the last height with a tile-row schedule")
TALL_OFF = Case("16x4104", 16, 4104, reaches="513 tile rows: the first height without one")
TALLEST = Case("8x65535", 8, 65535, reaches="the tallest frame: the packed row | view << 16 at its largest")
TALLEST_SHARDED = Case("8x65535_16x2", 8, 65535, 16, 2, "the tallest frame in shards")
TOO_TALL = Case("8x65536", 8, 65536, reaches="refused")
WIDE = Case("70003x3", 70003, 3, reaches="x / W beyond 16 bits")
DEINTERLEAVE = [Case("2048x1100_16x3", 2048, 1100, 16, 3), Case("2048x1100_12x5", 2048, 1100, 12, 5)]

WORLD = ("GEN_INT_TERRAIN", 128, 128, 128, 16)
HIT_MIX = dict(shadow=1, bounce_samples=2, bounce_all_hits=1)  # the ray kinds of the sharded cases


# ---- the oracle ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(vxo):
    return vxo.World.generate(getattr(vxo, WORLD[0]), *WORLD[1:])


def stale_pattern(shape, dtype, seed):
    """a buffer's contents before a launch: random bytes for the frame, negative indices below the oracle's -1 for the hit
    AOV, and finite floats no shading produces for the colour AOV and the history"""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 255, size=shape, dtype=np.uint8)
    if dtype == np.int64:
        return rng.integers(-1000, -2, size=shape, dtype=np.int64)
    return (-1000.0 - rng.integers(0, 1 << 20, size=shape)).astype(np.float32)


def params(vxo, case, cam, mode, **kw):
    cb, fn = MODES[mode]
    pos, f, u, r = helpers.camera(cam, world(vxo).dims, vxo) if isinstance(cam, str) else cam
    kw.setdefault("frame_number", fn)
    return vxo.make_params(case.W, case.H, pos, f, u, r, checkerboard=cb, **kw)


_FULL = {}


def oracle_full(vxo, case, cam, mode, **kw):
    """the oracle's full frame (fb over zeros, colour, hit, stats), computed once per key and left unchanged"""
    key = (case.W, case.H, cam, mode, tuple(sorted(kw.items())))
    if key not in _FULL:
        r = world(vxo).render(params(vxo, case, cam, mode, **kw), fb=np.zeros((case.H, case.W, 4), np.uint8), want_color=True,
                              want_hit=True, nthreads=16)
        for k in ("fb", "color", "hit"):
            r[k].setflags(write=False)
        _FULL[key] = r
    return _FULL[key]


RAY_COUNTERS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_hits")
PROBE_COUNTERS = ("coarse_probes", "brick_entries", "fine_probes")
_SHARD_STATS = {}


def oracle_shard_stats(vxo, case, cam, mode, shard, **kw):
    """the ray and probe counters of a shard: the sum over the oracle's renders of its strips (row_begin, row_end)"""
    key = (case.name, cam, mode, shard, tuple(sorted(kw.items())))
    if key not in _SHARD_STATS:
        tot = dict.fromkeys(RAY_COUNTERS + PROBE_COUNTERS + ("pixels_written",), 0)
        for b, e in case.strips_of(shard):
            st = world(vxo).render(params(vxo, case, cam, mode, row_begin=b, row_end=e, **kw), nthreads=16)["stats"]
            for k in RAY_COUNTERS + ("pixels_written",):
                tot[k] += int(getattr(st, k))
            for k in PROBE_COUNTERS:
                tot[k] += int(getattr(st.probes, k))
        _SHARD_STATS[key] = tot
    return _SHARD_STATS[key]
