"""Timing probe of surface extraction (vxrt_extract_surface), for profiles/r13_surface.md.

A 512 x 256 x 512 window of the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) placed at the
terrain surface, VXRT_SURF_CAP.  Timed on the stream with device events, the median of 20 calls after 3 warm-up calls, each
on a workspace and outputs allocated once: vxrt_read_region of the halo box (the floor: the call contains it), the counting
call (capacity 0), the extraction without triangles and the extraction with them.  Prints the summary, the quads per face
and the bytes each call writes.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times.

usage: python tools/surface_probe.py [--dims 512,256,512] [--mode 0]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(torch, fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="512,256,512")
    ap.add_argument("--mode", type=int, default=0)
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    dims = tuple(int(v) for v in a.dims.split(","))
    ctx = vx.Context(0)
    ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
    ox, oz = 4000, 3000
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    origin = (ox, max(int(np.median(heights)) - dims[1] // 2, 0), oz)
    L, h = ctx._L, ctx._h
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    s = torch.cuda.current_stream().cuda_stream
    halo_o, halo_d = tuple(v - 1 for v in origin), tuple(v + 2 for v in dims)
    bits = torch.empty(vx.region_words(halo_d), dtype=torch.int32, device="cuda")
    work = torch.empty(ctx.surface_workspace_bytes(dims), dtype=torch.uint8, device="cuda")
    summ = torch.zeros(16, dtype=torch.int32, device="cuda")
    first = ctx.extract_surface(origin, dims, a.mode).summary
    n = first.quads
    quads = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    verts = torch.empty((4 * n, 3), dtype=torch.int32, device="cuda")
    tris = torch.empty((2 * n, 3), dtype=torch.int32, device="cuda")

    def read():
        vx._native.check(L.vxrt_read_region(h, i3(halo_o), i3(halo_d), bits.data_ptr(), s))

    def extract(cap, tri):
        vx._native.check(L.vxrt_extract_surface(h, i3(origin), i3(dims), a.mode, work.data_ptr(), quads.data_ptr() if cap else None, cap,
                                                verts.data_ptr() if tri else None, tris.data_ptr() if tri else None, summ.data_ptr(), s))

    print("window origin %s dims %s mode %d workspace %d bytes" % (origin, dims, a.mode, work.numel()))
    print("summary", first, "quads per face %.4f" % (n / max(first.faces, 1)))
    t_read = _timed(torch, read)
    print("read_region of the halo box    median %.3f ms (min %.3f max %.3f), %d bytes written" % (*t_read, bits.numel() * 4))
    for name, cap, tri, out in [("counting call (capacity 0)   ", 0, False, 64), ("extract, quads only          ", n, False, 64 + 8 * n),
                                ("extract, quads and triangles ", n, True, 64 + 80 * n)]:
        t = _timed(torch, lambda: extract(cap, tri))
        print("%s median %.3f ms (min %.3f max %.3f), %d bytes written, %.2f x read_region" % (name, *t, out, t[0] / t_read[0]))
    ctx.close()


if __name__ == "__main__":
    main()
