"""Timing probe of the neighbour-count voxel rules (vxrt_apply_rule), for profiles/r19_rule.md.

The bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) and one 256 x 128 x 256 window of it at the
terrain surface.  Timed on the stream with device events, the median of `--reps` calls after 3 warm-up calls, on a workspace
and outputs allocated once:

  copy     the stream copy, measured the way bench.py measures its roofline line's stream_copy_gbs
  light    one vxrt_light_field call, the sky channel: 14 rounds, the nearest existing yardstick (a round there reads 7 plane
           words per output word, a rule round up to 27)
  rule     vxrt_apply_rule with the majority tables of each neighbourhood, N6 / N18 / N26, at 1 and 4 iterations, in both
           scopes (BOX: halo 1; WORLD: halo = iterations)

A rule round's own time is (4 iterations - 1 iteration) / 3 in the BOX scope, where the halo does not grow with the
iterations; the light round's is the sky call's time over 14 (its set-up and read-out spread over the rounds: an upper
bound).  Both are printed per plane word of their halo, with their ratio.

usage: python tools/rule_probe.py [--reps 20] [--dims 256,128,256]
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


def _plane_words(dims, h):
    return ((dims[0] + 2 * h + 31) // 32) * (dims[1] + 2 * h) * (dims[2] + 2 * h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
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
    origin = (ox, max(int(np.median(heights)) - dims[1] // 2, 16), oz)
    L, h = ctx._L, ctx._h
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    s = torch.cuda.current_stream().cuda_stream
    nvox = dims[0] * dims[1] * dims[2]
    print("window origin %s dims %s" % (origin, dims))

    levels = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    lsum = torch.zeros(42, dtype=torch.int32, device="cuda")
    lwork = torch.empty(ctx.light_workspace_bytes(dims, 1), dtype=torch.uint8, device="cuda")
    t = _timed(torch, lambda: vx._native.check(L.vxrt_light_field(h, i3(origin), i3(dims), None, 0, 1, lwork.data_ptr(), levels.data_ptr(),
                                                                   lsum.data_ptr(), s)), reps=a.reps)
    light_round = 1e6 * t[0] / 14 / _plane_words(dims, 14)
    print("light  sky: median %.3f ms (min %.3f max %.3f); at most %.4f ns per plane word and round" % (*t, light_round))

    bits = torch.empty(vx.region_words(dims), dtype=torch.int32, device="cuda")
    rsum = torch.zeros(12, dtype=torch.int32, device="cuda")
    for nb, name in ((vx.RULE_N6, "N6"), (vx.RULE_N18, "N18"), (vx.RULE_N26, "N26")):
        n = vx.Rule.count(nb)
        med = {}
        for scope, sname in ((vx.RULE_BOX, "box"), (vx.RULE_WORLD, "world")):
            for it in (1, 4):
                rule = vx.Rule(nb, range(n // 2 + 1, n + 1), range(n // 2, n + 1), it, scope)
                desc = rule._c()
                work = torch.empty(ctx.rule_workspace_bytes(dims, rule), dtype=torch.uint8, device="cuda")

                def call():
                    vx._native.check(L.vxrt_apply_rule(h, i3(origin), i3(dims), C.byref(desc), None, work.data_ptr(), bits.data_ptr(),
                                                       rsum.data_ptr(), s))
                first = ctx.apply_rule(origin, dims, rule).summary
                t = _timed(torch, call, reps=a.reps)
                med[(sname, it)] = t[0]
                print("%-3s %-5s %d iterations: median %.3f ms (min %.3f max %.3f); %.4f ns per voxel and iteration; workspace %d bytes"
                      % (name, sname, it, *t, 1e6 * t[0] / nvox / it, work.numel()))
                print("         summary %s" % (first,))
        per_round = (med[("box", 4)] - med[("box", 1)]) / 3
        per_word = 1e6 * per_round / _plane_words(dims, 1)
        print("%-3s round: %.1f us = %.4f ns per voxel = %.4f ns per plane word; %.2f x the light round's bound"
              % (name, 1e3 * per_round, 1e6 * per_round / nvox, per_word, per_word / light_round))
    ctx.close()


if __name__ == "__main__":
    main()
