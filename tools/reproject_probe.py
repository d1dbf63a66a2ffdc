"""Timing probe of the temporal filter (vxrt_reproject_frame), for profiles/reproject.md.

The bench frame with a moving camera: the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) at
1920 x 1080 with shadow and one bounce sample; each of the four bench cameras is rendered at two poses a step and a slight
turn apart, the first frame's history (a call without history) is the second frame's input.  Timed on the stream with device
events, the median of `--reps` calls after 3 warm-up calls, on buffers allocated once, the variants alternating:

  full        history, colour, BGRA8 and summary
  no summary  history, colour and BGRA8 (no memset, no atomics)
  no fb       history and colour
  bare        history only
  first       a call without history (no taps)
  copy        a device-to-device copy of W * H * 34 bytes: 68 bytes moved per pixel, what a full call reads (12 colour, 4 key,
              one 16-byte record and one 4-byte key for the taps, which neighbouring lanes largely share) and writes
              (16 + 12 + 4), the floor of a call

usage: python tools/reproject_probe.py [--reps 30] [--width 1920] [--height 1080] [--profile]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAMERAS = [("A", (0.50, 0.90, 0.50), (-0.45, 0.70, 0.0)), ("B", (0.10, 1.20, 0.10), (-0.60, 3.90, 0.0)),
           ("C", (0.50, 1.50, 0.50), (-1.5707, 0.0, 0.0)), ("D", (0.02, 0.55, 0.50), (-0.05, 1.5707, 0.0))]
STEP, TURN = (3.0, -0.5, 2.0), (0.005, 0.01, 0.0)


def _timed_alternating(torch, fns, warm=3, reps=30):
    """{name: (median, min, max) in ms}: one call of every variant per repetition, in turn"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--profile", action="store_true", help="camera A only: three full calls, then three without summary, untimed -- the run to put under rocprofv3")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    W, H = a.width, a.height
    ctx = vx.Context(0)
    X, Y, Z = 8192, 512, 8192
    ctx.build_world(vx.GEN_PERLIN_REF, X, Y, Z, 32)
    light = float(np.float32(1.0) / np.sqrt(np.float32(3.0), dtype=np.float32))
    ctx.SetEnvironment((light, light, light), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.zeros((H, W), dtype=torch.int64, device="cuda")
    keys = [torch.zeros(H * W, dtype=torch.int32, device="cuda") for _ in range(2)]
    hist = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    out = torch.zeros_like(col)
    src = torch.zeros(W * H * 34, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    print("frame %d x %d, library %s" % (W, H, os.environ.get("VXRT_LIB", "libvxrt.so")))
    for name, frac, euler in CAMERAS[:1] if a.profile else CAMERAS:
        cams = []
        for j in range(2):
            f, u, r = vx.GetDirections(tuple(e + j * t for e, t in zip(euler, TURN)))
            cams.append((tuple(fr * d + j * s for fr, d, s in zip(frac, (X, Y, Z), STEP)), f, u, r))
        ctx.RenderScreen(W, H, fb, *cams[0], vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=1), color_aov=col, hit_aov=hit)
        ctx.frame_guides(W, H, *cams[0], hit, out=keys[0])
        ctx.reproject_frame(col, keys[0], cams[0], cams[0], out_history=hist[0], out=out, summary=False)
        ctx.RenderScreen(W, H, fb, *cams[1], vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=2), color_aov=col, hit_aov=hit)
        ctx.frame_guides(W, H, *cams[1], hit, out=keys[1])
        kw = dict(history=hist[0], prev_keys=keys[0], out_history=hist[1])
        call = lambda **more: ctx.reproject_frame(col, keys[1], cams[1], cams[0], **more)
        s = call(out=out, fb=fb, **kw).summary
        print("camera %s: hit %d reused %d offscreen %d rejected %d" % (name, *s))
        if a.profile:
            for _ in range(3):
                call(out=out, fb=fb, **kw)
            for _ in range(3):
                call(out=out, fb=fb, summary=False, **kw)
            torch.cuda.synchronize()
            break
        t = _timed_alternating(torch, {
            "copy": lambda: dst.copy_(src),
            "full": lambda: call(out=out, fb=fb, **kw),
            "no summary": lambda: call(out=out, fb=fb, summary=False, **kw),
            "no fb": lambda: call(out=out, summary=False, **kw),
            "bare": lambda: ctx._L.vxrt_reproject_frame(ctx._h, W, H, col.data_ptr(), keys[1].data_ptr(), hist[0].data_ptr(),
                                                        keys[0].data_ptr(), _params(vx, cams), hist[1].data_ptr(), None, None, None,
                                                        torch.cuda.current_stream().cuda_stream),
            "first": lambda: call(out=out, fb=fb, out_history=hist[1]),
        }, reps=a.reps)
        for k, (med, lo, hi) in t.items():
            print("  %-10s median %.1f us (min %.1f max %.1f) = %.2f x copy" % (k, med * 1e3, lo * 1e3, hi * 1e3, med / t["copy"][0]))
    ctx.close()


def _params(vx, cams):
    import ctypes as C
    from voxelengine_amd import _native as N
    p = N.ReprojectParams(struct_size=C.sizeof(N.ReprojectParams), ortho=0, max_history=32)
    for pose, cam in ((p.cur, cams[1]), (p.prev, cams[0])):
        pose.origin, pose.fwd, pose.up, pose.right = ((C.c_float * 3)(*[float(x) for x in v]) for v in cam)
    return C.byref(p)


if __name__ == "__main__":
    main()
