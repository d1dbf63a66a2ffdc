"""Box collision query costs on the bench world (include/vxrt.h, vxrt_move_boxes / vxrt_overlap_boxes), one MI355X: the
median wall time of one call plus a stream synchronisation for
  * 1, 1k, 64k and 1M small bodies (0.6 x 1.8 x 0.6 voxels, |delta| <= 1 per axis) spread over the world's surface band;
  * 64k bodies of 16^3 voxels with |delta| = 16 on every axis;
  * the overlap query on the same inputs.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`; `--summary DIR` prints the median duration
per kernel and grid size of such a run's kernel_trace.csv.
usage: python3 tools/collide_probe.py [--out FILE.json] [--reps 20]
       python3 tools/collide_probe.py --summary ROCPROF_OUTPUT_DIR"""
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
            if "k_move_boxes" not in name and "k_overlap_boxes" not in name:
                continue
            grid = r.get("Grid_Size_X", r.get("Grid_Size", "?"))
            rows[(name.split("(")[0], grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid), us in sorted(rows.items(), key=lambda kv: (kv[0][0], int(kv[0][1]) if kv[0][1].isdigit() else 0)):
        print("%-24s grid %-10s n=%-3d median %10.1f us  min %10.1f us" % (name, grid, len(us), statistics.median(us), min(us)))


def bodies(rng, n, ext, dmax, dims, surface):
    """n bodies of extent `ext` whose centres lie in the band of +-24 voxels around the terrain surface"""
    x = rng.uniform(0, dims[0] - ext[0], n)
    z = rng.uniform(0, dims[2] - ext[2], n)
    ix = np.clip((x / 32).astype(int), 0, surface.shape[0] - 1)
    iz = np.clip((z / 32).astype(int), 0, surface.shape[1] - 1)
    y = np.clip(surface[ix, iz] + rng.uniform(-24, 24, n), 0, dims[1] - ext[1])
    lo = np.stack([x, y, z], 1)
    d = rng.uniform(-dmax, dmax, (n, 3)) if dmax < 16 else rng.choice([-dmax, dmax], (n, 3))
    return np.concatenate([lo, lo + np.asarray(ext), d], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
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
    ctx.build_world(gen, X, Y, Z, F)
    ctx.synchronize()
    # the surface height per 32 x 32 column: the highest non-empty brick row (from the coarse bits, no pool download)
    d = ctx.download_world(with_pool=False)
    cx, cy, cz = (int(c) for c in d["cdims"])
    occ = d["brick_slot"] != vx.EMPTY_SLOT
    # tiled cell order of the C ABI: tile (8^3 cells) index x-fastest, then cell within the tile x-fastest
    t = np.arange(occ.size)
    tile, cell = t // 512, t % 512
    tx, ty, tz = tile % (cx // 8), (tile // (cx // 8)) % (cy // 8), tile // ((cx // 8) * (cy // 8))
    bx, by, bz = tx * 8 + cell % 8, ty * 8 + (cell // 8) % 8, tz * 8 + cell // 64
    top = np.full((cx, cz), 0, np.int64)
    np.maximum.at(top, (bx[occ], bz[occ]), by[occ] + 1)
    surface = top * F
    res = {"world": [X, Y, Z], "factor": F, "runs": []}
    rng = np.random.default_rng(1)
    runs = [("small", n, (0.6, 1.8, 0.6), 1.0) for n in (1, 1024, 65536, 1 << 20)] + [("large", 65536, (16, 16, 16), 16.0)]
    for kind, n, ext, dmax in runs:
        b = torch.from_numpy(bodies(rng, n, ext, dmax, (X, Y, Z), surface)).cuda()
        entry = {"bodies": kind, "n": n, "extent": list(ext), "max_delta": dmax}
        for q in ("move", "overlap"):
            call = (lambda: ctx.move_boxes(b)) if q == "move" else (lambda: ctx.overlap_boxes(b))
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            entry[q + "_us_median"] = round(statistics.median(ts), 1)
            entry[q + "_us_min"] = round(min(ts), 1)
            if q == "move":
                fl = out[1].cpu().numpy()
                entry["blocked_fraction"] = round(float(np.count_nonzero(fl & 7)) / n, 4)
            else:
                entry["mean_overlap"] = round(float(out[0].double().mean()), 3)
        res["runs"].append(entry)
        print(json.dumps(entry), flush=True)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
