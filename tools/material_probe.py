"""Timing probe of the voxel materials (vxrt_material_frame, vxrt_material_field), for profiles/material.md.

Frames: one rendered bench frame per camera -- the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device)
at --width x --height with shadow and one bounce sample, its guide keys -- under three altitude bands and a six-tile 8 x 8
atlas.  Timed on the stream with device events around BATCH = 10 calls through the C ABI, the median over `--reps` such
batches after 3 warm-up batches divided by BATCH, on buffers allocated once, the variants alternating:

  atlas        vxrt_material_frame with atlas, colour, BGRA8 and summary
  no atlas     the same without an atlas (no texel load)
  bare         with atlas, colour only (no memset, no atomics: one 64 x 4 tile per workgroup)
  light        vxrt_light_frame without levels on the same frame with colour, BGRA8 and summary: the yardstick
  copy         a device-to-device copy of W * H * 40 bytes

Fields: vxrt_material_field on a 128^3 box and on a 512 x 128 x 512 window at the terrain surface, one call each per batch
entry, against vxrt_read_region of the same box.

usage: python tools/material_probe.py [--reps 30] [--width 1920] [--height 1080] [--cameras ABCD]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.reproject_probe import CAMERAS, _timed_alternating  # noqa: E402

BATCH = 10
BANDS = ((None, 1, 2, 3, 3), (300, 4, 5, 6, 0), (380, 7, 8, 9, 15))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cameras", default="ABCD")
    a = ap.parse_args()
    import torch
    import voxelengine_amd as vx
    from voxelengine_amd import _native as N
    W, H = a.width, a.height
    ctx = vx.Context(0)
    X, Y, Z = 8192, 512, 8192
    ctx.build_world(vx.GEN_PERLIN_REF, X, Y, Z, 32)
    light = float(np.float32(1.0) / np.sqrt(np.float32(3.0), dtype=np.float32))
    ctx.SetEnvironment((light, light, light), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    rules = vx.MaterialRules(BANDS)
    rng = np.random.default_rng(1)
    pal = vx.Palette(atlas=rng.integers(0, 256, (6, 8, 8, 4), dtype=np.uint8))
    for m in range(1, 10):
        pal.set(m, tint=(0.9, 0.8, 0.7), top=m % 6, side=(m + 1) % 6, bottom=(m + 2) % 6)
    d_pal = torch.from_numpy(pal.entries().view(np.int32)).cuda()
    d_atlas = torch.from_numpy(pal.atlas_words().view(np.int32)).cuda()
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    col = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.zeros((H, W), dtype=torch.int64, device="cuda")
    keys = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(col)
    src = torch.zeros(W * H * 40, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    summary = torch.zeros(4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    L = ctx._L
    print("frame %d x %d, library %s" % (W, H, os.environ.get("VXRT_LIB", "libvxrt.so")))
    r = rules._c()
    for name, frac, euler in CAMERAS:
        if name not in a.cameras:
            continue
        f, u, rt = vx.GetDirections(euler)
        cam = (tuple(fr * d for fr, d in zip(frac, (X, Y, Z))), f, u, rt)
        ctx.RenderScreen(W, H, fb, *cam, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=1), color_aov=col, hit_aov=hit)
        ctx.frame_guides(W, H, *cam, hit, out=keys)
        s = ctx.material_frame(col, keys, hit, cam, rules, pal, out=out, fb=fb).summary
        print("camera %s: hit %d painted %d top %d textured %d" % (name, *s))
        p = N.MaterialFrameParams(struct_size=C.sizeof(N.MaterialFrameParams), n_tiles=6, tile_shift=3)
        p.cam.origin, p.cam.fwd, p.cam.up, p.cam.right = ((C.c_float * 3)(*[float(x) for x in v]) for v in cam)
        lp = N.LightFrameParams(struct_size=C.sizeof(N.LightFrameParams), flags=3, outside_level=0xF0, sky_floor=0.25)
        lp.block_color, lp.ao_curve = (C.c_float * 3)(1.0, 0.8, 0.5), (C.c_float * 4)(0.4, 0.6, 0.8, 1.0)
        lp.cam = p.cam
        lp.box_origin, lp.box_dims = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)

        def material(atlas, full):
            for _ in range(BATCH):
                L.vxrt_material_frame(ctx._h, W, H, col.data_ptr(), keys.data_ptr(), hit.data_ptr(), C.byref(r), None, d_pal.data_ptr(),
                                      d_atlas.data_ptr() if atlas else None, C.byref(p), out.data_ptr(), fb.data_ptr() if full else None, None,
                                      summary.data_ptr() if full else None, stream)

        def lit():
            for _ in range(BATCH):
                L.vxrt_light_frame(ctx._h, W, H, col.data_ptr(), keys.data_ptr(), hit.data_ptr(), None, C.byref(lp), out.data_ptr(),
                                   fb.data_ptr(), None, summary.data_ptr(), stream)

        def copy():
            for _ in range(BATCH):
                dst.copy_(src)

        t = _timed_alternating(torch, {"copy": copy, "atlas": lambda: material(True, True), "no atlas": lambda: material(False, True),
                                       "bare": lambda: material(True, False), "light": lit}, reps=a.reps)
        for k, (med, lo, hi) in t.items():
            print("  %-10s median %.1f us (min %.1f max %.1f) = %.2f x light"
                  % (k, med * 1e3 / BATCH, lo * 1e3 / BATCH, hi * 1e3 / BATCH, med / t["light"][0]))

    # the fields: at the terrain surface under camera A
    column = ctx.read_region_host((4096, 0, 4096), (32, 512, 32))
    top = int(np.median(np.where(column.any(1), 511 - np.argmax(column[:, ::-1, :], axis=1), 0)))
    for dims in ((128, 128, 128), (512, 128, 512)):
        origin = (4096 - dims[0] // 2, max(top - dims[1] * 3 // 4, 0), 4096 - dims[2] // 2)
        n = dims[0] * dims[1] * dims[2]
        mats = torch.zeros(n, dtype=torch.uint8, device="cuda")
        fsum = torch.zeros(260, dtype=torch.int32, device="cuda")
        bits = torch.zeros(vx.region_words(dims), dtype=torch.int32, device="cuda")
        o3, d3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims)
        s = ctx.material_field(origin, dims, rules).summary
        print("field %s at %s: solid %d top %d" % (dims, origin, s.solid, s.top))

        def field():
            for _ in range(BATCH):
                L.vxrt_material_field(ctx._h, o3, d3, C.byref(r), None, mats.data_ptr(), fsum.data_ptr(), stream)

        def read():
            for _ in range(BATCH):
                L.vxrt_read_region(ctx._h, o3, d3, bits.data_ptr(), stream)

        t = _timed_alternating(torch, {"read_region": read, "field": field}, reps=a.reps)
        for k, (med, lo, hi) in t.items():
            print("  %-12s median %.1f us (min %.1f max %.1f) = %.2f x read_region"
                  % (k, med * 1e3 / BATCH, lo * 1e3 / BATCH, hi * 1e3 / BATCH, med / t["read_region"][0]))
    ctx.close()


if __name__ == "__main__":
    main()
