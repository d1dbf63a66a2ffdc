"""Timing probe of navigation fields (vxrt_nav_field), for profiles/r09_nav.md.

Windows of the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) placed at the terrain surface, and
a snake corridor (tests/ref_nav.snake_world, 256 x 8 x 128 cells, more than 16 000 levels).  For each case: the median wall
time of `n` calls, each one nav_field call (dist on, default agent) plus torch.cuda.synchronize(); the summary (levels,
tile_visits of tiles_total).  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times.

usage: python tools/nav_probe.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(ctx, torch, vx, origin, dims, goals, n):
    ctx.nav_field(origin, dims, goals, vx.NavAgent())  # warm: allocations, first launch
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = ctx.nav_field(origin, dims, goals, vx.NavAgent())
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), r.summary


def _report(name, t, s):
    print("%-28s wall %10.1f us  nodes %d goals %d reached %d levels %d tile_visits %d of %d tiles (%.2f per level)"
          % (name, t * 1e6, s.nodes, s.goals_used, s.reached, s.levels, s.tile_visits, s.tiles_total,
             s.tile_visits / max(s.levels, 1)), flush=True)


def main():
    import torch
    import voxelengine_amd as vx
    from oracle import vxo
    from tests import ref_nav
    ctx = vx.Context(0)
    ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
    ox, oz = 3500, 3500
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    y0 = max(int(np.median(heights)) - 40, 0)
    rng = np.random.default_rng(0)
    for name, d, ngoals in [("bench 256x64x256, 1 goal", (256, 64, 256), 1), ("bench 1024x128x1024, 1 goal", (1024, 128, 1024), 1),
                            ("bench 1024x128x1024, 1024 goals", (1024, 128, 1024), 1024)]:
        o = (ox, y0, oz)
        walk = vx.unpack_region(ctx.nav_field(o, d, [], vx.NavAgent()).walkable.cpu().numpy().view(np.uint32), d)
        p = np.argwhere(walk)
        goals = p[rng.choice(len(p), ngoals, replace=False)] + np.asarray(o)
        t, s = _time(ctx, torch, vx, o, d, goals, 5)
        _report(name, t, s)
    ctx.close()
    ctx = vx.Context(0)
    snake = ref_nav.snake_world(256, 128)
    v = np.zeros((256, 64, 128), bool)
    v[:, :snake.shape[1]] = snake
    w = vxo.World.from_voxels(v, 8)
    ctx.upload_world(w.factor, w.cdims, w.coarse_bits, w.brick_slot, w.bounds, w.pool)
    t, s = _time(ctx, torch, vx, (0, 0, 0), snake.shape, [(0, 1, 0)], 3)
    _report("snake 256x8x128", t, s)
    print("snake: %.2f us of wall time per level" % (t * 1e6 / s.levels), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
