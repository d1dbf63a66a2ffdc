"""Timing probe of the frame denoiser (vxrt_frame_guides, vxrt_denoise_frame), for profiles/denoise.md.

The bench frame: the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) at 1920 x 1080 with shadow
and one bounce sample, the four bench cameras.  Timed on the stream with device events, the median of `--reps` calls after 3
warm-up calls, on buffers allocated once:

  render   one single-view render launch of the bench frame with both AOVs, per camera (what a frame costs without filter)
  guides   vxrt_frame_guides
  n = 1 .. 5   vxrt_denoise_frame with n iterations, BGRA8 output included.  Iteration i of a call moves the same bytes
           whatever its role (16 read per tap, 16 written: float3 + BGRA8, or one record), so t(n) - t(n - 1) is the cost of
           the iteration at step 2^(n-1), and t(1) the cost of the iteration at step 1.
  copy     a device-to-device copy of W * H * 16 bytes (one record read and one written per pixel: W * H * 32 bytes moved),
           the floor of an iteration

With the A/B library (VXRT_LIB=.../libvxrt_exp.so) the calls are timed with VXRT_DENOISE_STAGED = 0 (every step DIRECT), 1
(step 1 STAGED), 2 (step 2 STAGED) and 3 (both), alternating within one run, and the outputs of the four are compared bit for
bit.  Kernel times come from a run of this probe under `rocprofv3 --kernel-trace --stats` with `--reps 3`.

usage: python tools/denoise_probe.py [--reps 30] [--width 1920] [--height 1080] [--color-scale 0.75] [--profile]
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


def _timed(torch, fn, warm=3, reps=30):
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--color-scale", type=float, default=0.75)
    ap.add_argument("--profile", action="store_true", help="camera A only: one render, one guides call and three 5-iteration "
                    "calls per colour scale, untimed -- the run to put under rocprofv3")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    W, H = a.width, a.height
    exp = "exp" in os.path.basename(os.environ.get("VXRT_LIB", ""))
    ctx = vx.Context(0)
    X, Y, Z = 8192, 512, 8192
    ctx.build_world(vx.GEN_PERLIN_REF, X, Y, Z, 32)
    light = float(np.float32(1.0) / np.sqrt(np.float32(3.0), dtype=np.float32))
    ctx.SetEnvironment((light, light, light), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.zeros((H, W), dtype=torch.int64, device="cuda")
    keys = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(col)
    work = torch.zeros(ctx.denoise_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    opts = vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=1)
    print("frame %d x %d, workspace %d bytes, library %s" % (W, H, work.numel(), os.environ.get("VXRT_LIB", "libvxrt.so")))
    if a.profile:
        name, frac, euler = CAMERAS[0]
        f, u, r = vx.GetDirections(euler)
        cam = ((frac[0] * X, frac[1] * Y, frac[2] * Z), f, u, r)
        ctx.RenderScreen(W, H, fb, *cam, opts, color_aov=col, hit_aov=hit)
        ctx.frame_guides(W, H, *cam, hit, out=keys)
        for scale in (0.0, a.color_scale):
            for _ in range(3):
                ctx.denoise_frame(col, keys, 5, scale, out=out, fb=fb, work=work)
        torch.cuda.synchronize()
        ctx.close()
        return
    src = torch.zeros(W * H * 16, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t = _timed(torch, lambda: dst.copy_(src), reps=a.reps)
    print("copy     median %.1f us (min %.1f max %.1f): %d bytes moved, %.0f GB/s" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, 2 * src.numel(),
                                                                                   2 * src.numel() / t[0] / 1e6))
    copy_us = t[0] * 1e3
    for name, frac, euler in CAMERAS:
        f, u, r = vx.GetDirections(euler)
        cam = ((frac[0] * X, frac[1] * Y, frac[2] * Z), f, u, r)
        t = _timed(torch, lambda: ctx.RenderScreen(W, H, fb, *cam, opts, color_aov=col, hit_aov=hit), reps=a.reps)
        render_us = t[0] * 1e3
        print("camera %s: render   median %.1f us (min %.1f max %.1f)" % (name, render_us, t[1] * 1e3, t[2] * 1e3))
        t = _timed(torch, lambda: ctx.frame_guides(W, H, *cam, hit, out=keys), reps=a.reps)
        k = keys.cpu().numpy().view(np.uint32)
        print("  guides   median %.1f us (min %.1f max %.1f); %d hit pixels, %d faces" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3,
                                                                                         int((k != 0).sum()), len(np.unique(k))))
        for scale in (0.0, a.color_scale):
            results = {}
            for mask in ((0, 1, 2, 3) if exp else (None,)):
                if mask is not None:
                    os.environ["VXRT_DENOISE_STAGED"] = str(mask)
                prev = 0.0
                for n in range(1, 6):
                    t = _timed(torch, lambda: ctx.denoise_frame(col, keys, n, scale, out=out, fb=fb, work=work), reps=a.reps)
                    us = t[0] * 1e3
                    print("  color_scale %.2f staged-mask %s n = %d: median %.1f us (min %.1f max %.1f); step %2d costs %.1f us = %.2f x copy, "
                          "%.3f of the render" % (scale, mask, n, us, t[1] * 1e3, t[2] * 1e3, 1 << (n - 1), us - prev, (us - prev) / copy_us,
                                                  (us - prev) / render_us))
                    prev = us
                results[mask] = out.clone()
            ref = results[0 if exp else None]
            for mask, got in results.items():
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), mask
            os.environ.pop("VXRT_DENOISE_STAGED", None)
    ctx.close()


if __name__ == "__main__":
    main()
