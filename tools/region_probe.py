"""Region readback and voxel stamp costs on the bench world (include/vxrt.h, vxrt_read_region / vxrt_edit_stamps), one
MI355X:
  * reads: wall time per vxrt_read_region call (launch + stream synchronisation) for 64^3, 256^3, 1024 x 512 x 1024 and the
    whole world, with the bytes the read moves computed from shapes (pool rows of the non-empty bricks in the window plus
    the words written) and the achieved rate;
  * stamps: a 64^3 ball brush in each mode at the terrain surface, and a 2048 x 512 x 2048 replace with an all-zero mask
    (the same voxels as the 2048 x 512 x 2048 box clear of tools/edit_probe.py);
  * undo of the r = 48 sphere brush: read of its bounding box, the edit, the replace stamp.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`; `--summary DIR` prints the median duration
per kernel and grid size of such a run's kernel_trace.csv.
usage: python3 tools/region_probe.py [--out FILE.json] [--reps 10]
       python3 tools/region_probe.py --summary ROCPROF_OUTPUT_DIR"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(d):
    rows = defaultdict(list)
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Kernel_Name", "")
            if not any(k in name for k in ("k_read_region", "k_stamp_bricks", "k_edit_bricks", "k_edit_commit")):
                continue
            grid = "%s x %s" % (r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Grid_Size_Y", "1"))
            rows[(name.split("(")[0], grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid), us in sorted(rows.items()):
        print("%-28s grid %-22s n=%-3d median %10.1f us  min %10.1f us" % (name, grid, len(us), statistics.median(us), min(us)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summary", default=None)
    args = ap.parse_args()
    if args.summary:
        summary(args.summary)
        return
    import torch
    import voxelengine_amd as vx
    from bench import WORKLOADS

    X, Y, Z, F, gen, W, H, shadow, bounce = WORKLOADS["c3_8k_1080p_shadow_bounce"]
    ctx = vx.Context(0)
    info = ctx.build_world(gen, X, Y, Z, F)
    ctx.synchronize()
    res = {"world": [X, Y, Z], "factor": F, "bricks": int(info.nslots)}
    d = ctx.download_world(with_pool=False)
    cx, cy, cz = d["cdims"]
    # occupancy of every cell in (x, y, z) order, decoded from the tiled cell order of the download
    t = np.arange(cx * cy * cz, dtype=np.int64)
    tile, inner = t >> 9, t & 511
    bx = (tile % (cx // 8)) * 8 + (inner & 7)
    by = ((tile // (cx // 8)) % (cy // 8)) * 8 + ((inner >> 3) & 7)
    bz = (tile // ((cx // 8) * (cy // 8))) * 8 + (inner >> 6)
    occ = np.zeros((cx, cy, cz), bool)
    occ[bx, by, bz] = d["brick_slot"] != 0xFFFFFFFF
    rng = np.random.default_rng(0)

    def surface(n):
        o = np.stack([rng.uniform(512, X - 512, n), np.full(n, Y - 0.5), rng.uniform(512, Z - 512, n)], 1).astype(np.float32)
        dd = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (n, 1))
        g = ctx.Raytrace(o, dd)
        return g["hitPoint"][g["hit"].astype(bool)].astype(np.int64)

    def wall(fn, reps):
        us = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        return round(statistics.median(us), 1), round(min(us), 1)

    reads = []
    for dims, origin in [((64, 64, 64), None), ((256, 256, 256), None), ((1024, 512, 1024), (2048, 0, 2048)),
                         ((X, Y, Z), (0, 0, 0))]:
        if origin is None:
            p = surface(1)[0]
            origin = tuple(int(v) // 32 * 32 - dd // 2 for v, dd in zip(p, dims))
            origin = (origin[0], max(min(origin[1], Y - dims[1]), 0), origin[2])
        out = torch.empty(vx.region_words(dims), dtype=torch.int32, device="cuda")
        ctx.read_region(origin, dims, out)       # first call: code load
        med, mn = wall(lambda: ctx.read_region(origin, dims, out), args.reps if dims[0] < X else 3)
        lo = [max(o, 0) // F for o in origin]
        hi = [-(-min(o + dd, n) // F) for o, dd, n in zip(origin, dims, (X, Y, Z))]
        live = int(occ[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].sum())
        moved = live * F ** 3 // 8 + vx.region_words(dims) * 4
        reads.append({"dims": list(dims), "origin": list(origin), "words": vx.region_words(dims), "live_bricks": live,
                      "bytes_moved": moved, "us_median": med, "us_min": mn,
                      "tb_per_s_at_median": round(moved / (med * 1e-6) / 1e12, 2)})
        del out
    res["reads"] = reads

    stamps = []
    g = np.indices((64, 64, 64)).astype(np.float64) - 31.5
    ball = (g ** 2).sum(0) <= 32.0 ** 2
    dball = torch.from_numpy(vx.pack_region(ball).view(np.int32)).cuda()
    ctx.edit_stamps([vx.Stamp((0, 0, 0), dball, vx.STAMP_UNION, (64, 64, 64))])   # first call: scratch, code load
    for mode, name in ((vx.STAMP_REPLACE, "replace"), (vx.STAMP_UNION, "union"), (vx.STAMP_SUBTRACT, "subtract")):
        us, touched = [], []
        for p in surface(args.reps):
            o = tuple(int(v) - 32 for v in p)
            t0 = time.perf_counter()
            st = ctx.edit_stamps([vx.Stamp(o, dball, mode, (64, 64, 64))])
            us.append((time.perf_counter() - t0) * 1e6)
            touched.append(int(st.bricks_touched))
        stamps.append({"stamp": "64^3 ball, %s" % name, "bricks_touched_median": int(statistics.median(touched)),
                       "us_median": round(statistics.median(us), 1), "us_min": round(min(us), 1), "calls": len(us)})
    big = (2048, 512, 2048)
    zero = torch.zeros(vx.region_words(big), dtype=torch.int32, device="cuda")
    us, touched = [], []
    for k in range(3):
        x0 = 1024 + 2048 * k
        t0 = time.perf_counter()
        st = ctx.edit_stamps([vx.Stamp((x0, 0, 2048), zero, vx.STAMP_REPLACE, big)])
        us.append((time.perf_counter() - t0) * 1e6)
        touched.append(int(st.bricks_touched))
    stamps.append({"stamp": "2048x512x2048 replace, all-zero mask", "bricks_touched_median": int(statistics.median(touched)),
                   "us_median": round(statistics.median(us), 1), "us_min": round(min(us), 1), "calls": len(us)})
    del zero
    res["stamps"] = stamps

    steps = defaultdict(list)
    for p in surface(args.reps):
        c = tuple(int(v) for v in p)
        o, dims = tuple(v - 48 for v in c), (97, 97, 97)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        saved = ctx.read_region(o, dims)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.edit_voxels([vx.EditSphere(c, 48, 0)])
        t2 = time.perf_counter()
        ctx.edit_stamps([vx.Stamp(o, saved, vx.STAMP_REPLACE, dims)])
        t3 = time.perf_counter()
        steps["read"].append((t1 - t0) * 1e6)
        steps["edit"].append((t2 - t1) * 1e6)
        steps["stamp"].append((t3 - t2) * 1e6)
    res["undo_sphere_r48"] = {k: round(statistics.median(v), 1) for k, v in steps.items()}
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
