"""Timing probe of mesh voxelization (vxrt_voxelize_mesh), for profiles/r11_voxelize.md.

Three workloads in each of the modes surface, solid and both: an icosphere of 20 480 triangles and radius 200 voxels in a
448^3 region, one of 81 920 triangles and radius 400 in an 832^3 region, and a soup of 10^4 triangles of about 1.5 voxels in
160 x 100 x 130.  The mesh is on the device, the workspace and the output are allocated once.  For each case: 2 warm-up calls,
then 10 calls, each ending in torch.cuda.synchronize(); the median, the least and the greatest wall time, the median of the
same calls bracketed by device events, and the summary.  For the icospheres also the yardstick of what touching that many
voxels costs here: one vxrt_edit_voxels sphere of the same radius set into (and cleared from) a 1024^3 world, and one
vxrt_read_region of the same box.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times.

usage: python tools/voxelize_probe.py [--skip-large]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(torch, call, n=10, warm=2):
    wall, dev = [], []
    for k in range(n + warm):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            wall.append(time.perf_counter() - t)
            dev.append(e0.elapsed_time(e1) / 1e3)
    return float(np.median(wall)) * 1e3, min(wall) * 1e3, max(wall) * 1e3, float(np.median(dev)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    from tests import ref_voxelize as R
    ctx = vx.Context(0)
    L, h = ctx._L, ctx._h
    cases = [("icosphere 20480, r 200", R.icosphere((224.0,) * 3, 200.0, 5), (448, 448, 448), 200)]
    if not a.skip_large:
        cases.append(("icosphere 81920, r 400", R.icosphere((416.0,) * 3, 400.0, 6), (832, 832, 832), 400))
    cases.append(("soup 10000", R.soup(10000, (160, 100, 130), 1.5, 1), (160, 100, 130), 0))
    have_world = False
    for name, (v, t), dims, radius in cases:
        dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda()
        ws = ctx.voxelize_workspace_bytes(dims, len(t))
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        out = torch.empty(vx.region_words(dims), dtype=torch.int32, device="cuda")
        summ = torch.zeros(8, dtype=torch.int32, device="cuda")
        d3 = (C.c_int32 * 3)(*dims)
        for modes, mname in [(1, "surface"), (2, "solid"), (3, "both")]:
            call = lambda: vx._native.check(L.vxrt_voxelize_mesh(h, dv.data_ptr(), len(v), dt.data_ptr(), len(t), d3, modes,
                                                                 work.data_ptr(), out.data_ptr(), summ.data_ptr(), None))
            med, lo, hi, dev = _timed(torch, call)
            s = summ.cpu().numpy().view(np.uint32)
            print("%-24s %-7s wall %8.3f ms (%.3f .. %.3f)  events %8.3f ms  set %d surface %d solid %d  workspace %.1f MiB"
                  % (name, mname, med, lo, hi, dev, s[0], s[1], s[2], ws / 2 ** 20), flush=True)
        if radius:
            if not have_world:
                ctx.build_world(vx.GEN_INT_TERRAIN, 1024, 1024, 1024, 32)
                have_world = True
            origin = tuple(512 - d // 2 for d in dims)  # the sphere and the box in the middle of the world
            times = {0: [], 1: []}
            for k in range(8):  # set, clear, set, ..: a call that changes nothing would write nothing
                torch.cuda.synchronize()
                tt = time.perf_counter()
                ctx.edit_voxels([vx.EditSphere((512, 512, 512), radius, 1 - k % 2)])
                times[1 - k % 2].append(time.perf_counter() - tt)
            buf = torch.empty(vx.region_words(dims), dtype=torch.int32, device="cuda")
            med, lo, hi, dev = _timed(torch, lambda: ctx.read_region(origin, dims, out=buf))
            print("%-24s yardstick: edit_voxels sphere set %.3f ms, clear %.3f ms (medians of 4, the first call left out: %s); "
                  "read_region of the box wall %.3f ms (%.3f .. %.3f), events %.3f ms"
                  % (name, np.median(times[1][1:]) * 1e3, np.median(times[0][1:]) * 1e3,
                     "%.3f ms" % (times[1][0] * 1e3), med, lo, hi, dev), flush=True)
        del work, out
    ctx.close()


if __name__ == "__main__":
    main()
