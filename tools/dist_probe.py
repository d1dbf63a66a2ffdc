"""Timing probe of exact distance fields (vxrt_distance_field), for profiles/r10_dist.md.

A 512 x 256 x 512 window of the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) placed at the
terrain surface, at R = 16, 64 and 255 in both modes.  For each case: the median wall time of 10 calls after 2 warm-up
calls, each one vxrt_distance_field call on a workspace and an output allocated once, ending in torch.cuda.synchronize(); the
same bracketed by device events; the summary; the tiles the empty-space skip filled (read from the workspace's last
section); and the bytes the sweeps must move at the least -- the halo's bits read once, each cell of the field after the y
sweep written and read once, two bytes per output voxel -- over the event time, as a share of a measured stream copy (a
1 GiB device-to-device copy, read + write, as bench.py measures it).  With --cpu, the same field by
tests/ref_dist.distance_field_scipy on 16 processes, each taking a slab of the box along z with its own halo (R = 255: 4
processes, for the memory of the transform's index arrays).  Run it under `rocprofv3 --kernel-trace --stats` (without --cpu)
for the per-kernel times.

usage: python tools/dist_probe.py [--cpu] [--radii 16,64,255]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS = (512, 256, 512)


def _stream_copy_gbs(torch):
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * n * 5 / (e0.elapsed_time(e1) / 1e3) / 1e9


def _min_bytes(d, r):
    h = [v + 2 * r for v in d]
    return (h[0] + 31) // 32 * h[1] * h[2] * 4 + 2 * 2 * d[0] * d[1] * h[2] + 2 * d[0] * d[1] * d[2]


def _slab(args):
    from tests import ref_dist
    world, z0, th, dims, radius, mode = args
    r = ref_dist.distance_field_scipy(world, (radius, radius, radius), (dims[0], dims[1], th), radius, mode)
    return z0, r["dist2"]


def _cpu(ctx, origin, dims, radius, mode, procs):
    """the field by the scipy restatement on `procs` processes (slabs along z, each with its halo); seconds, field"""
    import multiprocessing as mp
    th = dims[2] // procs
    jobs = []
    for k in range(procs):
        z0 = k * th
        o = (origin[0] - radius, origin[1] - radius, origin[2] + z0 - radius)
        world = ctx.read_region_host(o, (dims[0] + 2 * radius, dims[1] + 2 * radius, th + 2 * radius))
        jobs.append((world, z0, th, dims, radius, mode))
    t = time.perf_counter()
    with mp.get_context("spawn").Pool(procs) as pool:  # spawn: a child must not inherit this process's GPU state
        parts = pool.map(_slab, jobs)
    dt = time.perf_counter() - t
    out = np.empty(dims, np.uint16)
    for z0, p in parts:
        out[:, :, z0:z0 + th] = p
    return dt, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--radii", default="16,64,255")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    ctx = vx.Context(0)
    L, h = ctx._L, ctx._h
    ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
    copy_gbs = _stream_copy_gbs(torch)
    print("stream copy %.0f GB/s" % copy_gbs, flush=True)
    ox, oz = 3500, 3500
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    origin = (ox, max(int(np.median(heights)) - 128, 0), oz)
    print("window origin", origin, "dims", DIMS, flush=True)
    n = DIMS[0] * DIMS[1] * DIMS[2]
    out = torch.empty(n, dtype=torch.int16, device="cuda")
    summ = torch.zeros(6, dtype=torch.int32, device="cuda")
    o3, d3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*DIMS)
    tiles = (DIMS[0] // 64) * (DIMS[1] // 64) * (DIMS[2] // 64)
    for radius in [int(v) for v in a.radii.split(",")]:
        ws = ctx.distance_workspace_bytes(DIMS, radius)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        for mode, name in [(vx.DIST_TO_SOLID, "to_solid"), (vx.DIST_TO_EMPTY, "to_empty")]:
            call = lambda: vx._native.check(L.vxrt_distance_field(h, o3, d3, radius, mode, work.data_ptr(), out.data_ptr(),
                                                                   summ.data_ptr(), None))
            wall, dev = [], []
            for k in range(12):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t = time.perf_counter()
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                if k >= 2:
                    wall.append(time.perf_counter() - t)
                    dev.append(e0.elapsed_time(e1) / 1e3)
            w, d = float(np.median(wall)), float(np.median(dev))
            s = summ.cpu().numpy().view(np.uint32)
            live = int(work[ws - (tiles + 255) // 256 * 256:][:tiles].sum().item())
            mb = _min_bytes(DIMS, radius)
            print("R %3d %-8s wall %9.3f ms  events %9.3f ms  zero %d near %d far %d max_d2 %d sum_d2 %d  workspace %.1f MiB  "
                  "tiles filled %d of %d  least bytes %.1f MB = %.1f %% of the stream copy over the event time"
                  % (radius, name, w * 1e3, d * 1e3, s[0], s[1], s[2], s[3], int(s[4]) | int(s[5]) << 32, ws / 2 ** 20,
                     tiles - live, tiles, mb / 1e6, 100.0 * mb / d / 1e9 / copy_gbs), flush=True)
            if a.cpu:
                t, ref = _cpu(ctx, origin, DIMS, radius, mode, 16 if radius <= 64 else 4)
                got = out.cpu().numpy().view(np.uint16).reshape(DIMS[::-1]).transpose(2, 1, 0)
                print("R %3d %-8s scipy restatement on %d processes %.2f s = %.0f x the device call; fields equal: %s"
                      % (radius, name, 16 if radius <= 64 else 4, t, t / w, bool(np.array_equal(got, ref))), flush=True)
        del work
    ctx.close()


if __name__ == "__main__":
    main()
