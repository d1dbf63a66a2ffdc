"""Timing probe of the occupancy LOD (vxrt_downsample_region, Context.lod_world), for profiles/r14_lod.md.

The bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device).  At every shift 1 .. 5, two boxes: one z slab
of the whole-volume LOD (a source box of 8192 x 512 x 1024 voxels, the 2^32 limit of one call: the world is eight of them)
and a 512^3 window at the terrain surface.  Timed on the stream with device events, the median of `--reps` calls after 3
warm-up calls, each on a workspace and outputs allocated once:

  read     vxrt_read_region of the source box alone (the call contains it)
  bits     vxrt_downsample_region without counts
  counts   vxrt_downsample_region with counts
  reduce   bits - read and counts - read: the reduce pass by difference, which also holds the summary's fill and the gap
           between the launches.  The kernels' own times come from a run under `rocprofv3 --kernel-trace` with one box
           (`--boxes slab` or `--boxes window`), so that a kernel name stands for one shape: k_read_region and each
           instantiation of k_lod_reduce are then listed separately.
  whole    the eight slabs of the whole volume, eight calls between one pair of events (bits only)

with the bytes the reduce pass moves (the source words read once, the bits and counts written) over its time, and that rate
as a fraction of the stream copy measured here the way bench.py measures its roofline line's stream_copy_gbs (a 1 GiB
device-to-device copy, bytes read plus bytes written).  With the A/B library (VXRT_LIB=.../libvxrt_exp.so) the shifts that
have a SPLIT kernel (3 .. 5) are also timed with VXRT_LOD_SPLIT=0, the plain kernel, and VXRT_LOD_SPLIT=1, the SPLIT one.
Last, Context.lod_world end to end at every shift, stamps included (host clock around a device synchronise).

usage: python tools/lod_probe.py [--reps 20] [--shifts 1,2,3,4,5] [--boxes both|slab|window] [--no-world]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shifts", default="1,2,3,4,5")
    ap.add_argument("--boxes", default="both", choices=["both", "slab", "window"])
    ap.add_argument("--no-world", action="store_true", help="skip the lod_world end-to-end part")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    shifts = [int(v) for v in a.shifts.split(",")]
    exp = "exp" in os.path.basename(os.environ.get("VXRT_LIB", ""))
    ctx = vx.Context(0)
    ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
    copy = _stream_copy_gbs(torch)
    print("stream copy %.1f GB/s (1 GiB device to device, read + write)" % copy)
    ox, oz = 4000, 3000
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    win_o = (ox, max(int(np.median(heights)) - 256, 0), oz)
    L, h = ctx._L, ctx._h
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    s = torch.cuda.current_stream().cuda_stream
    for shift in shifts:
        f = 1 << shift
        boxes = [("slab 8192x512x1024", (0, 0, 3072), (8192, 512, 1024)), ("window 512^3", win_o, (512, 512, 512))]
        for name, origin, src in [b for b in boxes if a.boxes == "both" or b[0].startswith(a.boxes)]:
            dims = tuple(v // f for v in src)
            ws = ctx.lod_workspace_bytes(dims, shift)
            work = torch.empty(ws, dtype=torch.uint8, device="cuda")
            bits = torch.empty(vx.region_words(dims), dtype=torch.int32, device="cuda")
            cnt = torch.empty(dims[0] * dims[1] * dims[2], dtype=torch.int16, device="cuda")
            summ = torch.zeros(8, dtype=torch.int32, device="cuda")

            def read():
                vx._native.check(L.vxrt_read_region(h, i3(origin), i3(src), work.data_ptr(), s))

            def down(counts):
                vx._native.check(L.vxrt_downsample_region(h, i3(origin), i3(dims), shift, 1, work.data_ptr(), bits.data_ptr(),
                                                          cnt.data_ptr() if counts else None, summ.data_ptr(), s))

            first = ctx.downsample(origin, dims, shift, 1).summary
            print("shift %d %s: origin %s cells %s workspace %d bytes, %s" % (shift, name, origin, dims, ws, first))
            t_read = _timed(torch, read, reps=a.reps)
            print("  read     median %.3f ms (min %.3f max %.3f), %d bytes written" % (*t_read, ws))
            variants = [("", None)] + ([(" VXRT_LOD_SPLIT=0", "0"), (" VXRT_LOD_SPLIT=1", "1")] if exp and shift >= 3 else [])
            for tag, env in variants:
                if env is not None:
                    os.environ["VXRT_LOD_SPLIT"] = env
                for what, counts in [("bits  ", False), ("counts", True)]:
                    t = _timed(torch, lambda: down(counts), reps=a.reps)
                    moved = ws + bits.numel() * 4 + (cnt.numel() * 2 if counts else 0)
                    red = t[0] - t_read[0]
                    rate = moved / (red / 1e3) / 1e9 if red > 0 else float("nan")
                    print("  %s%s median %.3f ms (min %.3f max %.3f); reduce by difference %.3f ms = %.2f x read, %d bytes moved, "
                          "%.1f GB/s = %.3f of the stream copy" % (what, tag, *t, red, red / t_read[0], moved, rate, rate / copy))
                os.environ.pop("VXRT_LOD_SPLIT", None)
            if name.startswith("slab"):
                def whole():
                    for z in range(8):
                        vx._native.check(L.vxrt_downsample_region(h, i3((0, 0, 1024 * z)), i3(dims), shift, 1, work.data_ptr(),
                                                                  bits.data_ptr(), None, summ.data_ptr(), s))
                print("  whole volume, eight slabs, bits: median %.3f ms (min %.3f max %.3f)" % _timed(torch, whole, reps=a.reps))
            del work, bits, cnt
    if not a.no_world:
        for shift in shifts:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lod = ctx.lod_world(shift)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            info = lod.world_info()
            print("lod_world shift %d: %.1f ms end to end (8 slabs, stamps included), LOD world %s cells of %d, %d bricks"
                  % (shift, 1e3 * (t1 - t0), tuple(info.cdims), info.factor, info.nslots))
            lod.close()
    ctx.close()


if __name__ == "__main__":
    main()
