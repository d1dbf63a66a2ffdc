"""Timing probe of the stamp orientations (vxrt_transform_stamp), for profiles/r20_transform.md.

A 1024^3 stamp (128 MiB of bits) and a 64^3 piece (32 KiB), random bits at density 0.3.  For each of the six axis
permutations, with and without a flip of destination x: the median of `--reps` calls after 3 warm-up calls, timed on the
stream with device events in batches of `--batch` calls (a 64^3 call is shorter than an event pair resolves), with and
without a summary.  GB/s counts the source words plus the destination words.  Beside each stands a hipMemcpyAsync device to
device of the destination's byte count (the same read + write traffic), timed the same way in the same process, and the ratio
of the two.

usage: python tools/transform_probe.py [--reps 20] [--batch 10] [--sizes 1024,64]
"""
import argparse
import ctypes as C
import itertools
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(torch, fn, batch, warm=3, reps=20):
    """median, min and max of the time of one call in ms, over `reps` batches of `batch` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / batch)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--sizes", default="1024,64")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    ctx = vx.Context(0)
    L, h = ctx._L, ctx._h
    s = torch.cuda.current_stream().cuda_stream
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    for edge in (int(v) for v in a.sizes.split(",")):
        sd = (edge, edge, edge)
        n = vx.region_words(sd)
        g = torch.Generator(device="cuda").manual_seed(edge)
        src = torch.zeros(n, dtype=torch.int32, device="cuda")
        for b in range(32):  # density 0.3 per bit
            src |= (torch.rand(n, device="cuda", generator=g) < 0.3).to(torch.int32) << b
        dst = torch.empty(n, dtype=torch.int32, device="cuda")
        summ = torch.zeros(8, dtype=torch.int32, device="cuda")
        gb = 2.0 * 4 * n / 1e9
        print("stamp %d^3: %d words each way, %.3f MB moved per call" % (edge, n, 1e3 * gb))

        def copy():  # torch copies a contiguous tensor to one of the same type on the same device with hipMemcpyAsync
            dst.copy_(src)

        for axis in itertools.permutations((0, 1, 2)):
            for flip in (0, 1):
                desc = vx.Orientation(axis, flip)._c()
                row = []
                for with_summary in (False, True):
                    def call():
                        vx._native.check(L.vxrt_transform_stamp(h, src.data_ptr(), i3(sd), C.byref(desc), dst.data_ptr(),
                                                                summ.data_ptr() if with_summary else None, s))
                    t = _timed(torch, call, a.batch, reps=a.reps)
                    c = _timed(torch, copy, a.batch, reps=a.reps)  # the yardstick beside every figure
                    row.append((t, c))
                (t0, c0), (t1, c1) = row
                print("axis %s flip %d: %8.4f ms %7.1f GB/s (min %.4f max %.4f) | with summary %8.4f ms %7.1f GB/s | copy %8.4f ms %7.1f GB/s "
                      "| ratio to copy %.2f, with summary %.2f"
                      % (axis, flip, t0[0], gb / t0[0] * 1e3, t0[1], t0[2], t1[0], gb / t1[0] * 1e3, c0[0], gb / c0[0] * 1e3, t0[0] / c0[0], t1[0] / c1[0]))
        del src, dst
    ctx.close()


if __name__ == "__main__":
    main()
