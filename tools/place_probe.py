"""Voxel piece query costs on the bench world (include/vxrt.h, vxrt_place_pieces), one MI355X, beside the box queries on the
same integer boxes: the median wall time of one call plus a stream synchronisation for
  (a) 64k placements of a full 16^3 piece swept 16 along one axis (y, then x), and vxrt_move_boxes on the same 64k bodies with
      the same one-axis delta;
  (b) 1M fits (dist 0) of a full 1 x 2 x 1 piece, and vxrt_overlap_boxes on the same boxes;
  (c) one 256^3 piece of density 0.05 dropped 64 from above the terrain.
The results of (a) and (b) are compared with the box queries' before anything is timed.  Kernel times come from a separate
run under `rocprofv3 --kernel-trace --stats`; `--summary DIR` prints the median duration per kernel and grid size of such a
run's kernel_trace.csv.
usage: python3 tools/place_probe.py [--out FILE.json] [--reps 20]
       python3 tools/place_probe.py --summary ROCPROF_OUTPUT_DIR"""
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
KERNELS = ("k_place_", "k_move_boxes", "k_overlap_boxes")


def summary(d):
    rows = defaultdict(list)
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Kernel_Name", "")
            if not any(k in name for k in KERNELS):
                continue
            grid = "%s x %s" % (r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Grid_Size_Y", "1"))
            rows[(name.split("(")[0], grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid), us in sorted(rows.items()):
        print("%-28s grid %-18s n=%-3d median %10.1f us  min %10.1f us" % (name, grid, len(us), statistics.median(us), min(us)))


def surface_heights(ctx, vx, F):
    """the surface height per F x F column: the highest non-empty brick row (from the cell table, no pool download)"""
    d = ctx.download_world(with_pool=False)
    cx, cy, cz = (int(c) for c in d["cdims"])
    occ = d["brick_slot"] != vx.EMPTY_SLOT
    t = np.arange(occ.size)  # tiled cell order of the C ABI: tiles of 8^3 cells x-fastest, cells within a tile x-fastest
    tile, cell = t // 512, t % 512
    tx, ty, tz = tile % (cx // 8), (tile // (cx // 8)) % (cy // 8), tile // ((cx // 8) * (cy // 8))
    bx, by, bz = tx * 8 + cell % 8, ty * 8 + (cell // 8) % 8, tz * 8 + cell // 64
    top = np.zeros((cx, cz), np.int64)
    np.maximum.at(top, (bx[occ], bz[occ]), by[occ] + 1)
    return top * F


def origins(rng, n, ext, dims, surface, F):
    """n integer origins of boxes of extent `ext` in the band of +-24 voxels around the terrain surface"""
    x = rng.integers(0, dims[0] - ext[0], n)
    z = rng.integers(0, dims[2] - ext[2], n)
    y = np.clip(surface[x // F, z // F] + rng.integers(-24, 25, n), 0, dims[1] - ext[1])
    return np.stack([x, y, z], 1).astype(np.int32)


def timed(torch, call, reps):
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return out, round(statistics.median(ts), 1), round(min(ts), 1)


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
    surface = surface_heights(ctx, vx, F)
    rng = np.random.default_rng(1)
    res = {"world": [X, Y, Z], "factor": F, "runs": []}

    def record(entry):
        res["runs"].append(entry)
        print(json.dumps(entry), flush=True)

    def piece_of(grid):
        return vx.Piece(torch.from_numpy(vx.pack_region(grid).view(np.int32)).cuda(), grid.shape)

    def placements(o, axis, dist):
        pl = np.zeros((len(o), 6), np.int32)
        pl[:, 1:4], pl[:, 4], pl[:, 5] = o, axis, dist
        return torch.from_numpy(pl).cuda()

    def bodies(o, ext, axis, dist):
        b = np.zeros((len(o), 9), np.float32)
        b[:, :3], b[:, 3:6] = o, o + np.asarray(ext, np.int32)
        b[:, 6 + axis] = dist
        return torch.from_numpy(b).cuda()

    # (a) 64k full 16^3 pieces swept 16 along one axis, beside move_boxes with the same one-axis delta
    n, ext = 65536, (16, 16, 16)
    o = origins(rng, n, ext, (X, Y, Z), surface, F)
    cube = piece_of(np.ones(ext, bool))
    for axis, dist in ((1, -16), (0, 16)):
        pl, b = placements(o, axis, dist), bodies(o, ext, axis, dist)
        got, p_med, p_min = timed(torch, lambda: ctx.place_pieces([cube], pl), args.reps)
        (lohi, flags), m_med, m_min = timed(torch, lambda: ctx.move_boxes(b), args.reps)
        got, lohi = got.cpu().numpy(), lohi.cpu().numpy()
        free = got[:, 0] == 0  # the two rules agree where the box overlaps nothing at the start
        assert np.array_equal((lohi[:, axis] - o[:, axis])[free], got[free, 1].astype(np.float32))
        record({"case": "a", "n": n, "piece": list(ext), "axis": axis, "dist": dist, "place_us_median": p_med, "place_us_min": p_min,
                "move_us_median": m_med, "move_us_min": m_min, "blocked_fraction": round(float(np.mean(got[:, 3] == 1)), 4),
                "overlapping_fraction": round(float(np.mean(~free)), 4)})

    # (b) 1M fits of a 1 x 2 x 1 piece, beside overlap_boxes
    n, ext = 1 << 20, (1, 2, 1)
    o = origins(rng, n, ext, (X, Y, Z), surface, F)
    small = piece_of(np.ones(ext, bool))
    pl, b = placements(o, 1, 0), bodies(o, ext, 1, 0)
    got, p_med, p_min = timed(torch, lambda: ctx.place_pieces([small], pl), args.reps)
    (counts, _), c_med, c_min = timed(torch, lambda: ctx.overlap_boxes(b), args.reps)
    assert torch.equal(got[:, 0], counts)
    record({"case": "b", "n": n, "piece": list(ext), "place_us_median": p_med, "place_us_min": p_min, "overlap_us_median": c_med,
            "overlap_us_min": c_min, "mean_overlap": round(float(counts.double().mean()), 3)})

    # (c) one 256^3 piece dropped 64 from above the terrain
    big = piece_of(rng.random((256, 256, 256), dtype=np.float32) < 0.05)
    top = int(surface[4000 // F: 4256 // F + 1, 3000 // F: 3256 // F + 1].max())
    pl = placements(np.asarray([[4000, min(top + 20, Y - 1), 3000]], np.int32), 1, -64)
    got, p_med, p_min = timed(torch, lambda: ctx.place_pieces([big], pl), args.reps)
    record({"case": "c", "n": 1, "piece": [256, 256, 256], "dist": -64, "place_us_median": p_med, "place_us_min": p_min,
            "result": got.cpu().numpy()[0].tolist()})
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
