"""Timing probe of the sky on frames (vxrt_sky_frame), for profiles/sky_frame.md.

Frames: the bench world (8192 x 512 x 8192 PERLIN_REF, f = 32, built on the device) at --width x --height with shadow and one
bounce sample and its guide keys, under three cameras: `miss` looks up from above the terrain (every pixel a miss, every pixel
under the cloud plane), `mixed` is the bench's grazing camera D (terrain below the horizon, sky above it), `hit` the bench's
top-down camera C (every pixel a hit).  Timed on the stream with device events around BATCH = 10 calls through the C ABI, the
median over `--reps` such batches after 3 warm-up batches divided by BATCH, on buffers allocated once, the variants
alternating:

  sky          vxrt_sky_frame with six octaves of cloud, colour, BGRA8 and summary
  sky bare     the same, colour only (no zeroing launch, no atomics: one 64 x 4 tile per workgroup)
  no clouds    without VXRT_SKY_CLOUDS, colour, BGRA8 and summary
  one octave   clouds of one octave, colour, BGRA8 and summary
  light        vxrt_light_frame without levels on the same frame with colour, BGRA8 and summary: a yardstick
  material     vxrt_material_frame with an atlas on the same frame with colour, BGRA8 and summary: a yardstick
  copy         a device-to-device copy of W * H * 32 bytes (what a full sky call moves at the most)

usage: python tools/sky_probe.py [--reps 30] [--width 1920] [--height 1080]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.material_probe import BANDS  # noqa: E402
from tools.reproject_probe import CAMERAS, _timed_alternating  # noqa: E402

BATCH = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
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
    src = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    summary = torch.zeros(8, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    L = ctx._L
    print("frame %d x %d, library %s" % (W, H, os.environ.get("VXRT_LIB", "libvxrt.so")))
    r = rules._c()
    by_name = {name: (frac, euler) for name, frac, euler in CAMERAS}
    up = ((0.5 * X, 0.9 * Y, 0.5 * Z), (0.1, 0.98, 0.15), (0.0, -0.15, 0.98), (1.0, 0.0, -0.1))
    views = [("miss", up)]
    for kind, name in (("mixed", "D"), ("hit", "C")):
        frac, euler = by_name[name]
        views.append((kind, (tuple(fr * d for fr, d in zip(frac, (X, Y, Z))),) + tuple(vx.GetDirections(euler))))
    for kind, cam in views:
        ctx.RenderScreen(W, H, fb, *cam, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=1), color_aov=col, hit_aov=hit)
        ctx.frame_guides(W, H, *cam, hit, out=keys)
        sky = vx.Sky(flags=vx.SKY_CLOUDS, octaves=6, cloud_y=2.0 * Y, sun_dir=(light, light, light))
        s = ctx.sky_frame(col, keys, cam, sky, out=out, fb=fb, summary=True).summary
        print("frame %s: miss %d hit %d ground %d sun %d cloud %d fogged %d" % (kind, *s))
        sp = {k: kw._c(cam) for k, kw in (("six", sky), ("none", vx.Sky(**dict(vars(sky), flags=0))), ("one", vx.Sky(**dict(vars(sky), octaves=1))))}
        mp = N.MaterialFrameParams(struct_size=C.sizeof(N.MaterialFrameParams), n_tiles=6, tile_shift=3)
        mp.cam = sp["six"].cam
        lp = N.LightFrameParams(struct_size=C.sizeof(N.LightFrameParams), flags=3, outside_level=0xF0, sky_floor=0.25)
        lp.block_color, lp.ao_curve = (C.c_float * 3)(1.0, 0.8, 0.5), (C.c_float * 4)(0.4, 0.6, 0.8, 1.0)
        lp.cam = sp["six"].cam
        lp.box_origin, lp.box_dims = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)

        def sky_call(which, full):
            for _ in range(BATCH):
                L.vxrt_sky_frame(ctx._h, W, H, col.data_ptr(), keys.data_ptr(), C.byref(sp[which]), out.data_ptr(), fb.data_ptr() if full else None,
                                 summary.data_ptr() if full else None, stream)

        def material():
            for _ in range(BATCH):
                L.vxrt_material_frame(ctx._h, W, H, col.data_ptr(), keys.data_ptr(), hit.data_ptr(), C.byref(r), None, d_pal.data_ptr(),
                                      d_atlas.data_ptr(), C.byref(mp), out.data_ptr(), fb.data_ptr(), None, summary.data_ptr(), stream)

        def lit():
            for _ in range(BATCH):
                L.vxrt_light_frame(ctx._h, W, H, col.data_ptr(), keys.data_ptr(), hit.data_ptr(), None, C.byref(lp), out.data_ptr(),
                                   fb.data_ptr(), None, summary.data_ptr(), stream)

        def copy():
            for _ in range(BATCH):
                dst.copy_(src)

        t = _timed_alternating(torch, {"copy": copy, "sky": lambda: sky_call("six", True), "sky bare": lambda: sky_call("six", False),
                                       "no clouds": lambda: sky_call("none", True), "one octave": lambda: sky_call("one", True), "light": lit,
                                       "material": material}, reps=a.reps)
        for k, (med, lo, hi) in t.items():
            print("  %-10s median %.1f us (min %.1f max %.1f) = %.2f x light, %.2f x material"
                  % (k, med * 1e3 / BATCH, lo * 1e3 / BATCH, hi * 1e3 / BATCH, med / t["light"][0], med / t["material"][0]))
    ctx.close()


if __name__ == "__main__":
    main()
