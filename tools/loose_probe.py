"""Timing probe of the loose voxels (vxrt_loose_step), for profiles/loose_step.md.

The bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) and windows of it at the terrain surface, the
loose layer a random fifth of the voxels of a slab 16 voxels thick in the upper half of the window (what is on a solid is
dropped by the call).  Timed on the stream with device events, the median of `--reps` calls after 3 warm-up calls, on a
workspace and buffers allocated once, out of place (the input is the same for every call):

  copy     the stream copy, measured the way bench.py measures its roofline line's stream_copy_gbs
  loose    vxrt_loose_step for sand and water at 1 and 16 steps on each window

A step's own time is (16 steps - 1 step) / 15; the rest of a call (the region read, the set-up and the output) is the 1-step
call less one step.  The bytes a pass must move: the plane it writes, and the three planes of its stencil (the layer it reads,
blocked, live) read once from HBM -- four planes; printed as a rate and as a fraction of the stream copy.

usage: python tools/loose_probe.py [--reps 20] [--dims 128,128,128 --dims 512,128,512]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rule_probe import _plane_words, _stream_copy_gbs, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dims", action="append")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    ctx = vx.Context(0)
    ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
    copy = _stream_copy_gbs(torch)
    print("stream copy %.1f GB/s (1 GiB device to device, read + write)" % copy)
    ox, oz = 4000, 3000
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    L, h = ctx._L, ctx._h
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    for spec in a.dims or ["128,128,128", "512,128,512"]:
        dims = tuple(int(v) for v in spec.split(","))
        origin = (ox, max(int(np.median(heights)) - dims[1] // 2, 16), oz)
        nvox = dims[0] * dims[1] * dims[2]
        plane = 4 * _plane_words(dims, 1)
        layer = np.zeros(dims, bool)
        y0 = dims[1] * 3 // 4
        layer[:, y0:y0 + 16, :] = rng.random((dims[0], min(16, dims[1] - y0), dims[2])) < 0.2
        inp = torch.from_numpy(vx.pack_region(layer).view(np.int32)).to("cuda")
        out = torch.empty_like(inp)
        summ = torch.zeros(12, dtype=torch.int32, device="cuda")
        work = torch.empty(ctx.loose_workspace_bytes(dims), dtype=torch.uint8, device="cuda")
        print("window origin %s dims %s: plane %d bytes, workspace %d bytes" % (origin, dims, plane, work.numel()))
        for material, name, per in ((vx.LOOSE_SAND, "sand", 2), (vx.LOOSE_WATER, "water", 3)):
            med = {}
            for steps in (1, 16):
                desc = vx.Loose(material, steps, vx.LOOSE_WALL, 0)._c()

                def call():
                    vx._native.check(L.vxrt_loose_step(h, i3(origin), i3(dims), C.byref(desc), inp.data_ptr(), work.data_ptr(), out.data_ptr(),
                                                       summ.data_ptr(), s))
                call()
                torch.cuda.synchronize()
                first = vx.engine.LooseResult(out, origin, dims, summ.clone(), s).summary
                t = _timed(torch, call, reps=a.reps)
                med[steps] = t[0]
                print("%-5s %2d steps: median %.3f ms (min %.3f max %.3f); %.4f ns per voxel and step" % (name, steps, *t, 1e6 * t[0] / nvox / steps))
                print("         summary %s" % (first,))
            step = (med[16] - med[1]) / 15
            fixed = med[1] - step
            gbs = per * 4 * plane / (step / 1e3) / 1e9
            print("%-5s step: %.1f us (%d passes, %.1f us each); read + set-up + output: %.1f us = %.0f %% of the 16-step call; "
                  "%d bytes per pass -> %.0f GB/s = %.2f of the stream copy"
                  % (name, 1e3 * step, per, 1e3 * step / per, 1e3 * fixed, 100 * fixed / med[16], 4 * plane, gbs, gbs / copy))
    ctx.close()


if __name__ == "__main__":
    main()
