"""Voxel edit costs on the bench world (include/vxrt.h, vxrt_edit_voxels), one MI355X:
  * wall time per edit call against bricks touched: spheres of radius 0 / 16 / 48 / 160 voxels at the terrain surface and a
    2048 x 512 x 2048 box clear (run under `rocprofv3 --kernel-trace --stats` for the k_edit_bricks / k_edit_commit share);
  * one pool growth by 1.5x (vxrt_edit_reserve: a new allocation and a copy of the live pool);
  * the bench frame rate (1080p, shadow + 1 bounce, one view per launch and 16 views per launch) after 1000 random brush
    edits -- new bricks land past the high-water mark, out of cell order -- against the same world after a save and reload
    (the compacting save renumbers the bricks in cell order).
usage: python3 tools/edit_probe.py [--out FILE.json] [--brushes 1000]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--brushes", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch

    import voxelengine_amd as vx
    from bench import CAMERAS, WORKLOADS

    X, Y, Z, F, gen, W, H, shadow, bounce = WORKLOADS["c3_8k_1080p_shadow_bounce"]
    ctx = vx.Context(0)
    t0 = time.perf_counter()
    info = ctx.build_world(gen, X, Y, Z, F)
    ctx.synchronize()
    res = {"world": [X, Y, Z], "factor": F, "build_s": round(time.perf_counter() - t0, 3), "bricks": int(info.nslots)}
    light = float(np.float32(1.0) / np.sqrt(np.float32(3.0)))
    ctx.SetEnvironment((light, light, light), (2, 2, 2), (0.5, 0.5, 0.5))
    ctx.SetFOV(90.0)
    rng = np.random.default_rng(0)

    def surface(n):
        o = np.stack([rng.uniform(0, X, n), np.full(n, Y - 0.5), rng.uniform(0, Z, n)], 1).astype(np.float32)
        d = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (n, 1))
        g = ctx.Raytrace(o, d)
        return g["hitPoint"][g["hit"].astype(bool)].astype(np.int64)

    def timed(ops):
        t = time.perf_counter()
        st = ctx.edit_voxels(ops)
        return (time.perf_counter() - t) * 1e6, st

    ctx.edit_voxels([vx.EditSphere((0, 0, 0), 0, 0)])  # first call: scratch allocation, code load
    lat = []
    for r in (0, 16, 48, 160):
        us, touched = [], []
        for k, p in enumerate(surface(10)[:10]):
            t, st = timed([vx.EditSphere(tuple(int(v) for v in p), r, k & 1)])
            us.append(t)
            touched.append(int(st.bricks_touched))
        lat.append({"shape": "sphere r=%d" % r, "bricks_touched_median": int(statistics.median(touched)),
                    "us_median": round(statistics.median(us), 1), "us_min": round(min(us), 1), "calls": len(us)})
    us, touched = [], []
    for k in range(3):
        x0 = 1024 + 2048 * k
        t, st = timed([vx.EditBox((x0, 0, 2048), (x0 + 2047, 511, 4095), 0)])
        us.append(t)
        touched.append(int(st.bricks_touched))
    lat.append({"shape": "box 2048x512x2048 clear", "bricks_touched_median": int(statistics.median(touched)),
                "us_median": round(statistics.median(us), 1), "us_min": round(min(us), 1), "calls": len(us)})
    res["latency"] = lat

    cap = int(ctx.edit_voxels([]).pool_capacity)
    t = time.perf_counter()
    ctx.edit_reserve(cap + (cap + 1) // 2)
    res["growth"] = {"capacity_before": cap, "capacity_after": cap + (cap + 1) // 2,
                     "ms": round((time.perf_counter() - t) * 1e3, 2), "pool_bytes_copied": int(ctx.world_info().nslots) * F ** 3 // 8}

    # 1000 brush edits, one call each
    pts = surface(args.brushes * 2)[: args.brushes]
    bus = []
    for k, p in enumerate(pts):
        t, st = timed([vx.EditSphere(tuple(int(v) for v in p), int(rng.integers(4, 25)), int(rng.integers(0, 2)))])
        bus.append(t)
    st = ctx.edit_voxels([])
    res["brushes"] = {"calls": len(bus), "us_median": round(statistics.median(bus), 1),
                      "us_p90": round(float(np.percentile(bus, 90)), 1), "pool_slots": int(st.pool_slots),
                      "bricks_live": int(st.bricks_live), "pool_capacity": int(st.pool_capacity)}

    cams = []
    for name, frac, euler in CAMERAS:
        f, u, r = vx.GetDirections(euler)
        cams.append(((frac[0] * X, frac[1] * Y, frac[2] * Z), f, u, r))
    frames = torch.zeros((16, H, W, 4), dtype=torch.uint8, device="cuda")

    def rate(V):
        opts = vx.RenderOptions(shadow=bool(shadow), bounce_samples=bounce)

        def step(i):
            if V == 1:
                for j in range(16):
                    pos, f, u, r = cams[(i * 16 + j) % len(cams)]
                    opts.frame_number = i * 16 + j + 1
                    ctx.RenderScreen(W, H, frames[j], pos, f, u, r, opts)
            else:
                views = []
                for j in range(16):
                    pos, f, u, r = cams[(i * 16 + j) % len(cams)]
                    views.append(dict(fb=frames[j], origin=pos, fwd=f, up=u, right=r, frame_number=i * 16 + j + 1))
                ctx.RenderViews(W, H, views, opts)
        for i in range(3):
            step(i)
        torch.cuda.synchronize()
        ctx.frame_stats()
        t = time.perf_counter()
        for i in range(args.steps):
            step(3 + i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        rays = ctx.frame_stats().total_rays()
        return {"views_per_launch": V, "frames_per_s": round(16 * args.steps / dt, 1), "mrays_per_s": round(rays / dt / 1e6, 1)}

    res["frames_after_brushes"] = [rate(1), rate(16)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "edited.vxb")
        t = time.perf_counter()
        ctx.save_world(path)
        save_s = time.perf_counter() - t
        t = time.perf_counter()
        info2 = ctx.load_world(path)
        res["save_reload"] = {"save_s": round(save_s, 2), "load_s": round(time.perf_counter() - t, 2), "nslots": int(info2.nslots)}
    res["frames_after_save_reload"] = [rate(1), rate(16)]
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
