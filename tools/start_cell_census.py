#!/usr/bin/env python3
"""Where do the tracer's walks start?  A CPU census with the Python transcription of the reference (oracle/ref_py.py), its
`dda` wrapped to record every walk: no GPU, no library.

usage: tools/start_cell_census.py [pixels per camera = 300] [X Y Z = 768 512 768] [brick edge = 32]

World: the `perlin_ref` generator (oracle/vxo.py), the bench's generator at a size the CPU builds in a minute.  Cameras A, C
and D at the bench's fractional poses (camera B starts outside the grid and looks past it), random pixels of a 1920 x 1080
frame at 90 degrees through a pinhole model (not the product's camera code: the census is about orders of magnitude).
Each pixel's chain as the shaded launch runs it: the primary ray; for a hit, the shadow ray from pos + 0.01 L along the
light and one bounce sample from pos + 0.01 n (a random direction of the hemisphere, max_steps = 8).

Printed per ray kind: coarse walks, coarse walks whose start cell is occupied, coarse walks that end at their first probe
with a tight-box hit (0 coarse steps), brick walks, brick walks that end at their first probe on a voxel.  These are the
starts the render kernel's probed set-up (csrc/vxrt_wave2.hpp: start_pending_probed) parks in the round that sets them up."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_py, vxo  # noqa: E402

CAMERAS = [("A", (0.50, 0.90, 0.50), (-0.45, 0.70, 0.0)), ("C", (0.50, 1.50, 0.50), (-1.5707, 0.0, 0.0)),
           ("D", (0.02, 0.55, 0.50), (-0.05, 1.5707, 0.0))]
WIDTH, HEIGHT = 1920, 1080
KINDS = ("primary", "shadow", "bounce")


def main():
    n_pix = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    X, Y, Z = (int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (768, 512, 768)
    factor = int(sys.argv[5]) if len(sys.argv) > 5 else 32
    t0 = time.time()
    w = vxo.World.generate(vxo.GEN_PERLIN_REF, X, Y, Z, factor, nthreads=os.cpu_count() or 8)
    world = ref_py.PyWorld(w.factor, w.cdims, w.coarse_bits, w.brick_slot, w.bounds, w.pool)
    print("world perlin_ref %d x %d x %d, brick edge %d: %d of %d coarse cells occupied (%.0f s)" % (
        X, Y, Z, factor, int((np.asarray(w.brick_slot) != 0xFFFFFFFF).sum()), int(np.prod(w.cdims)), time.time() - t0), flush=True)

    counts = {k: dict(rays=0, coarse=0, coarse_occupied=0, coarse_box_at_0=0, brick=0, brick_hit_at_0=0) for k in KINDS}
    kind = ["primary"]
    plain_dda = ref_py.dda

    def counting_dda(words, dims, start, d, events, per_cell_bounds=None, **kw):
        r = plain_dda(words, dims, start, d, events, per_cell_bounds=per_cell_bounds, **kw)
        c = counts[kind[0]]
        if per_cell_bounds is not None:  # a coarse walk
            c["coarse"] += 1
            cell = [ref_py.f2i(v) for v in start]
            if all(0 <= cell[a] < dims[a] for a in range(3)):
                c["coarse_occupied"] += ref_py.bit(words, ref_py.sample_index(cell[0], cell[1], cell[2], dims[0], dims[1]))
            c["coarse_box_at_0"] += int(r.hit and not r.oob and r.steps == 0)
        else:
            c["brick"] += 1
            c["brick_hit_at_0"] += int(r.hit and r.steps == 0)
        return r

    ref_py.dda = counting_dda
    try:
        f32 = np.float32
        light = np.full(3, f32(1.0) / np.sqrt(f32(3.0)), f32)
        rng = np.random.default_rng(18)
        k = np.tan(np.pi / 4)
        for name, frac, euler in CAMERAS:
            fwd, up, right = (np.asarray(v, np.float64) for v in vxo.get_directions(euler))
            pos = np.array([frac[0] * X, frac[1] * Y, frac[2] * Z], f32)
            for _ in range(n_pix):
                su, sv = rng.random() * 2 - 1, rng.random() * 2 - 1
                ray = (fwd + su * k * (WIDTH / HEIGHT) * right + sv * k * up).astype(f32)
                kind[0] = "primary"
                counts["primary"]["rays"] += 1
                p = ref_py.raytrace(world, pos, ray)
                if not p["hit"]:
                    continue
                at = np.asarray(p["pos"], f32)
                normal = -np.asarray(p["normal"], f32)
                kind[0] = "shadow"
                counts["shadow"]["rays"] += 1
                ref_py.raytrace(world, at + f32(0.01) * light, light)
                sd = (rng.random(3) * 2 - 1).astype(f32)
                sd /= np.linalg.norm(sd)
                if float(np.dot(sd, normal)) < 0:
                    sd = (sd - 2 * np.dot(sd, normal) * normal).astype(f32)
                kind[0] = "bounce"
                counts["bounce"]["rays"] += 1
                ref_py.raytrace(world, at + f32(0.01) * normal, sd, max_steps=8)
            print("camera %s done (%.0f s)" % (name, time.time() - t0), flush=True)
    finally:
        ref_py.dda = plain_dda

    total = {key: sum(counts[k][key] for k in KINDS) for key in counts["primary"]}
    pct = lambda a, b: "%5.1f %%" % (100.0 * a / b) if b else "    -"
    print("%-8s %7s %13s %16s %18s %12s %18s" % ("kind", "rays", "coarse walks", "start occupied", "box hit at step 0", "brick walks", "voxel at step 0"))
    for name, c in list(counts.items()) + [("all", total)]:
        print("%-8s %7d %13d %8d %s %9d %s %12d %9d %s" % (name, c["rays"], c["coarse"], c["coarse_occupied"], pct(c["coarse_occupied"], c["coarse"]),
                                                          c["coarse_box_at_0"], pct(c["coarse_box_at_0"], c["coarse"]), c["brick"],
                                                          c["brick_hit_at_0"], pct(c["brick_hit_at_0"], c["brick"])))
    print("coarse walks that start occupied, per ray: %.2f" % (total["coarse_occupied"] / max(total["rays"], 1)))


if __name__ == "__main__":
    main()
