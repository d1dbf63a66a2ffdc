"""Timing probe of voxel light fields (vxrt_light_field), for profiles/r16_light.md.

The bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) and one 256 x 128 x 256 window of it at the
terrain surface.  Timed on the stream with device events, the median of `--reps` calls after 3 warm-up calls, on a workspace
and outputs allocated once:

  read     vxrt_read_region of the halo box alone (the call contains it)
  sky      vxrt_light_field, the sky channel
  block    vxrt_light_field, the block channel with 4096 emitters (seeded: random voxels of the box, levels 1 .. 15)
  both     vxrt_light_field, both channels, the same emitters

with the bytes each call moves by the design's own model (`model_bytes` below: every plane word a launch reads or writes,
counted once per launch, neighbour loads that other lanes of the launch also make not counted again) and that volume over
the call's time as a fraction of the stream copy measured here the way bench.py measures its roofline line's
stream_copy_gbs (a 1 GiB device-to-device copy, bytes read plus bytes written).  The kernels' own times come from a run of
this probe under `rocprofv3 --kernel-trace --stats` with `--only sky|block|both`, so that a kernel name stands for one shape.

usage: python tools/light_probe.py [--reps 20] [--only all|sky|block|both] [--dims 256,128,256]
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


def _stream_copy_gbs(torch):
    nbytes = 1 << 30
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(5):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * 5 / (e0.elapsed_time(e1) / 1e3) / 1e9


def model_bytes(dims, channels, n_emitters):
    """the bytes one call moves, by the design's own model, as (total, parts)"""
    h = [d + 28 for d in dims]
    P = 4 * ((h[0] + 31) // 32) * h[1] * h[2]  # one bit plane of the halo box
    n = bin(channels).count("1")
    sky, block = channels & 1, channels >> 1 & 1
    nvox = dims[0] * dims[1] * dims[2]
    box_planes = P * dims[1] * dims[2] // (h[1] * h[2])  # the rows of a plane that hold voxels of B
    parts = {
        "halo read (plane written)": P,
        "columns (solid read, empty written, S_15 written)": 2 * P + sky * P,
        "block S_15 cleared": block * P,
        # a round reads S_k+1 and empty and writes S_k; the level planes are read and written where the carry is not 0:
        # counted here as all four planes both ways, the most a round can move
        "14 rounds (S read, empty read, S written)": 14 * n * 3 * P,
        "14 rounds (level planes, upper bound)": 14 * n * 8 * P,
        "emitters (classify, 15 scatters)": block * n_emitters * (16 + 8 + 15 * 8),
        "expand (planes of B read, bytes written)": n * 5 * box_planes + nvox,
        "tally (planes of B read)": (1 + n * 5) * box_planes,
    }
    return sum(parts.values()), parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="all", choices=["all", "sky", "block", "both"])
    ap.add_argument("--dims", default="256,128,256")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    dims = tuple(int(v) for v in a.dims.split(","))
    ctx = vx.Context(0)
    ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
    copy = _stream_copy_gbs(torch)
    print("stream copy %.1f GB/s (1 GiB device to device, read + write)" % copy)
    ox, oz = 4000, 3000
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    origin = (ox, max(int(np.median(heights)) - dims[1] // 2, 14), oz)
    rng = np.random.default_rng(16)
    em = np.stack([origin[k] + rng.integers(0, dims[k], 4096) for k in range(3)] + [rng.integers(1, 16, 4096)], 1).astype(np.int32)
    d_em = torch.from_numpy(em).cuda()
    L, h = ctx._L, ctx._h
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    s = torch.cuda.current_stream().cuda_stream
    nvox = dims[0] * dims[1] * dims[2]
    out = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    summ = torch.zeros(42, dtype=torch.int32, device="cuda")
    work = torch.empty(ctx.light_workspace_bytes(dims, 3), dtype=torch.uint8, device="cuda")
    print("window origin %s dims %s, workspace %d bytes (both channels)" % (origin, dims, work.numel()))
    if a.only == "all":
        ho, hd = tuple(v - 14 for v in origin), tuple(v + 28 for v in dims)
        t = _timed(torch, lambda: vx._native.check(L.vxrt_read_region(h, i3(ho), i3(hd), work.data_ptr(), s)), reps=a.reps)
        print("read   median %.3f ms (min %.3f max %.3f), halo %s" % (*t, hd))
    for name, channels in [("sky", 1), ("block", 2), ("both", 3)]:
        if a.only not in ("all", name):
            continue
        n = 4096 if channels & 2 else 0

        def call():
            vx._native.check(L.vxrt_light_field(h, i3(origin), i3(dims), d_em.data_ptr() if n else None, n, channels, work.data_ptr(),
                                                out.data_ptr(), summ.data_ptr(), s))
        first = ctx.light_field(origin, dims, em if n else None, channels).summary
        t = _timed(torch, call, reps=a.reps)
        total, parts = model_bytes(dims, channels, n)
        rate = total / (t[0] / 1e3) / 1e9
        print("%-6s median %.3f ms (min %.3f max %.3f); model %d bytes, %.1f GB/s = %.3f of the stream copy; %.2f ns per voxel"
              % (name, *t, total, rate, rate / copy, 1e6 * t[0] / nvox))
        for k, v in parts.items():
            if v:
                print("         %-52s %12d" % (k, v))
        print("         summary %s" % (first,))
    ctx.close()


if __name__ == "__main__":
    main()
