"""Timing probe of floating-island detection (vxrt_find_islands), for profiles/r08_islands.md.

Windows of the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) and a 256^3 random world at density
0.31 (near the site-percolation threshold of the cubic lattice, where components are largest and most tangled).  For each
case: the median wall time of 20 calls, each one find_islands call (labels off, table of 4096 rows) plus
torch.cuda.synchronize(); the summary.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times.

usage: python tools/islands_probe.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(ctx, torch, origin, dims, anchors, n=20):
    ctx.find_islands(origin, dims, anchors)  # warm: allocations, first launch
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = ctx.find_islands(origin, dims, anchors)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), r.summary


def main():
    import torch
    import voxelengine_amd as vx
    from oracle import vxo
    all_ = vx.ISLAND_ANCHOR_FACES | vx.ISLAND_ANCHOR_FLOOR
    ctx = vx.Context(0)
    ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
    cases = [("bench 64^3 brush", (4096, 192, 4096), (64, 64, 64), all_),
             ("bench 256^3", (4096, 128, 4096), (256, 256, 256), all_),
             ("bench 512^3", (4096, 0, 4096), (512, 512, 512), all_),
             ("bench 512^3 anchors=0", (4096, 0, 4096), (512, 512, 512), 0)]
    for name, o, d, a in cases:
        t, s = _time(ctx, torch, o, d, a)
        print("%-24s wall %9.1f us  components %d islands %d island_voxels %d" % (name, t * 1e6, *s), flush=True)
    ctx.close()
    ctx = vx.Context(0)
    v = np.random.default_rng(0).random((256, 256, 256)) < 0.31
    w = vxo.World.from_voxels(v, 32)
    ctx.upload_world(w.factor, w.cdims, w.coarse_bits, w.brick_slot, w.bounds, w.pool)
    for name, a in (("random 0.31 256^3", all_), ("random 0.31 256^3 anch=0", 0)):
        t, s = _time(ctx, torch, (0, 0, 0), (256, 256, 256), a)
        print("%-24s wall %9.1f us  components %d islands %d island_voxels %d" % (name, t * 1e6, *s), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
