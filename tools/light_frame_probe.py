"""Timing probe of the light on frames (vxrt_light_frame), for profiles/light_frame.md.

One rendered bench frame per camera: the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) at
1920 x 1080 with shadow and one bounce sample, its guide keys, and the light field of a 512 x 212 x 512 box in front of
camera A with two emitters.  Timed on the stream with device events around BATCH = 10 calls through the C ABI (its host side is
a few microseconds, so the stream stays fed), the median over `--reps` such batches after 3 warm-up batches divided by BATCH,
on buffers allocated once, the variants alternating:

  full           colour, BGRA8 and summary
  bare           colour only (no memset, no atomics: one 64 x 4 tile per workgroup)
  reproject      vxrt_reproject_frame on the same frame with history, colour, BGRA8 and summary: the yardstick
  copy           a device-to-device copy of W * H * 40 bytes: 80 bytes moved per pixel, what a full call reads of its own (12
                 colour, 4 key, 8 hit index) and writes (12 + 4), and as much again for what the nine cells cost at best

Each camera's line also gives the mean length of the runs of equal (hit index, key) along x: how many neighbouring pixels show
one face (profiles/light_frame.md has the form that shared a face's corners within such a run, and why it was dropped).

usage: python tools/light_frame_probe.py [--reps 30] [--width 1920] [--height 1080]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.reproject_probe import CAMERAS, STEP, TURN, _params, _timed_alternating  # noqa: E402

BATCH = 10
BOX = ((3840, 250, 3840), (512, 212, 512))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
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
    src = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    field = ctx.light_field(*BOX, [(4096, 440, 4096, 15), (4150, 420, 4200, 12)])
    print("frame %d x %d, library %s" % (W, H, os.environ.get("VXRT_LIB", "libvxrt.so")))
    print("light box", BOX, "summary", tuple(field.summary)[:2])

    for name, frac, euler in CAMERAS:
        cams = []
        for j in range(2):
            f, u, r = vx.GetDirections(tuple(e + j * t for e, t in zip(euler, TURN)))
            cams.append((tuple(fr * d + j * s for fr, d, s in zip(frac, (X, Y, Z), STEP)), f, u, r))
        ctx.RenderScreen(W, H, fb, *cams[0], vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=1), color_aov=col, hit_aov=hit)
        ctx.frame_guides(W, H, *cams[0], hit, out=keys[0])
        ctx.reproject_frame(col, keys[0], cams[0], cams[0], out_history=hist[0], out=out, summary=False)
        ctx.RenderScreen(W, H, fb, *cams[1], vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=2), color_aov=col, hit_aov=hit)
        ctx.frame_guides(W, H, *cams[1], hit, out=keys[1])

        s = ctx.light_frame(col, keys[1], hit, cams[1], field, out=out, fb=fb).summary
        keyed = keys[1].view(H, W)
        heads = int(((keyed[:, 1:] != keyed[:, :-1]) | (hit[:, 1:] != hit[:, :-1])).sum()) + H
        print("camera %s: hit %d in_box %d occluded %d dark %d; %.1f pixels per run of equal (hit, key) along x" % (name, *s, W * H / heads))
        import ctypes as C
        from voxelengine_amd import _native as N
        p = N.LightFrameParams(struct_size=C.sizeof(N.LightFrameParams), flags=3, outside_level=0xF0, sky_floor=0.25)
        p.block_color, p.ao_curve = (C.c_float * 3)(1.0, 0.8, 0.5), (C.c_float * 4)(0.4, 0.6, 0.8, 1.0)
        p.cam.origin, p.cam.fwd, p.cam.up, p.cam.right = ((C.c_float * 3)(*[float(x) for x in v]) for v in cams[1])
        p.box_origin, p.box_dims = (C.c_int32 * 3)(*BOX[0]), (C.c_int32 * 3)(*BOX[1])
        summary = torch.zeros(4, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        rp = _params(vx, cams)

        def batch(full):
            for _ in range(BATCH):
                ctx._L.vxrt_light_frame(ctx._h, W, H, col.data_ptr(), keys[1].data_ptr(), hit.data_ptr(), field.levels.data_ptr(), C.byref(p),
                                        out.data_ptr(), fb.data_ptr() if full else None, None, summary.data_ptr() if full else None, stream)

        def reproject():
            for _ in range(BATCH):
                ctx._L.vxrt_reproject_frame(ctx._h, W, H, col.data_ptr(), keys[1].data_ptr(), hist[0].data_ptr(), keys[0].data_ptr(), rp,
                                            hist[1].data_ptr(), out.data_ptr(), fb.data_ptr(), summary.data_ptr(), stream)

        def copy():
            for _ in range(BATCH):
                dst.copy_(src)

        t = _timed_alternating(torch, {"copy": copy, "full": lambda: batch(True), "bare": lambda: batch(False), "reproject": reproject},
                               reps=a.reps)
        for k, (med, lo, hi) in t.items():
            print("  %-10s median %.1f us (min %.1f max %.1f) = %.2f x copy"
                  % (k, med * 1e3 / BATCH, lo * 1e3 / BATCH, hi * 1e3 / BATCH, med / t["copy"][0]))
    ctx.close()


if __name__ == "__main__":
    main()
