"""Box collision queries on the device (include/vxrt.h, vxrt_move_boxes / vxrt_overlap_boxes): moves bit-equal to the
reference of tests/ref_collide.py (lo / hi compared as float bits, flags and counts equal) on random worlds at f = 8, 16
and 32 and a wide grid, after edits and stamps, on the bench world (against the reference on read_region_host windows), on
side streams, through the host wrapper and through the headless example's walk mode."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region, vxo_edit
from tests import helpers
from tests import ref_collide as R
from tests.helpers import eng, float_bits, gen_dense, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YXZ, XYZ = (1, 0, 2), (0, 1, 2)


def _world(vxo, size, factor, density, seed):
    """helpers.random_voxel_world and the bool grid it was made from (the same draw)"""
    w = helpers.random_voxel_world(vxo, size, factor, density, seed)
    vox = np.random.default_rng(seed).random(size) < density
    return w, vox


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _assert_move(vx, torch, ctx, vox, b, order=YXZ, origin=(0, 0, 0)):
    lohi, flags = ctx.move_boxes(_dev(torch, b), order)
    torch.cuda.synchronize()
    wl, wf = R.move_boxes(vox, b, order, origin)
    got = lohi.cpu().numpy()
    bad = np.flatnonzero((float_bits(got) != float_bits(wl)).any(1))
    assert len(bad) == 0, (len(bad), b[bad[:3]].tolist(), got[bad[:3]].tolist(), wl[bad[:3]].tolist())
    assert np.array_equal(flags.cpu().numpy().view(np.uint32), wf)
    return got, wf


def _assert_overlap(vx, torch, ctx, vox, b):
    counts, flags = ctx.overlap_boxes(_dev(torch, b))
    wc, wo = R.overlap_boxes(vox, b)
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), wc)
    assert np.array_equal(flags.cpu().numpy().view(np.uint32), wo)
    return wc


WORLDS = [(8, (64, 64, 64), 0.05), (16, (128, 128, 128), 0.03), (32, (256, 256, 256), 0.02), (8, (8192, 64, 64), 0.03)]


@pytest.mark.parametrize("factor,size,density", WORLDS)
def test_moves_and_counts_equal_the_reference(eng, vxo, factor, size, density):
    """~100k random bodies per world -- extents and steps at the limits, bodies half outside, invalid ones -- in two orders"""
    vx, torch = eng
    w, vox = _world(vxo, size, factor, density, seed=factor + size[0])
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        b = R.random_bodies(np.random.default_rng(size[0] + factor), size, 100_000)
        for order in (YXZ, XYZ):
            _, wf = _assert_move(vx, torch, ctx, vox, b, order)
            assert np.count_nonzero(wf & 7) > 5000 and np.count_nonzero(wf == R.INVALID) > 100
        assert _assert_overlap(vx, torch, ctx, vox, b).max() > 0
        # the host wrapper gives the device path's results
        lohi, flags = ctx.move_boxes(_dev(torch, b[:5000]))
        hl, hf = ctx.move_boxes(b[:5000])
        assert np.array_equal(float_bits(hl), float_bits(lohi.cpu().numpy()))
        assert np.array_equal(hf, flags.cpu().numpy().view(np.uint32))
        hc, ho = ctx.overlap_boxes(b[:5000])
        assert np.array_equal(hc, R.overlap_boxes(vox, b[:5000])[0]) and np.array_equal(ho, R.overlap_boxes(vox, b[:5000])[1])
        hl, hf = ctx.move_boxes([vx.Body((1, 1, 1), (2, 3, 2), (0, -1, 0))])
        assert np.array_equal(float_bits(hl), float_bits(R.move_boxes(vox, [[1, 1, 1, 2, 3, 2, 0, -1, 0]])[0]))
    finally:
        ctx.close()


def test_results_follow_edits_and_stamps(eng, vxo):
    vx, torch = eng
    w, vox = _world(vxo, (128, 128, 128), 16, 0.02, seed=7)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        b = R.random_bodies(np.random.default_rng(8), vox.shape, 50_000)
        before, _ = _assert_move(vx, torch, ctx, vox, b)
        ops = [(0, 1, (0, 40, 0), (127, 42, 127)), (1, 0, (64, 41, 64), (20, 0, 0)), (0, 0, (10, 0, 10), (30, 127, 30))]
        ctx.edit_voxels([vx.EditBox(a, bb, v) if k == 0 else vx.EditSphere(a, bb[0], v) for k, v, a, bb in ops])
        vox = ref_edit.apply_edits(vox, ops)
        after, _ = _assert_move(vx, torch, ctx, vox, b)
        assert not np.array_equal(float_bits(before), float_bits(after))
        _assert_overlap(vx, torch, ctx, vox, b)
        rng = np.random.default_rng(9)
        stamps = [((20, 60, 20), rng.random((50, 10, 70)) < 0.5, vx.STAMP_UNION),
                  ((-5, 30, 50), np.ones((60, 20, 40), bool), vx.STAMP_SUBTRACT),
                  ((70, 0, 0), rng.random((40, 100, 128)) < 0.1, vx.STAMP_REPLACE)]
        ctx.edit_stamps([vx.Stamp(o, m, mode) for o, m, mode in stamps])
        vox = ref_region.apply_stamps(vox, stamps)
        stamped, _ = _assert_move(vx, torch, ctx, vox, b)
        assert not np.array_equal(float_bits(stamped), float_bits(after))
        _assert_overlap(vx, torch, ctx, vox, b)
    finally:
        ctx.close()


def test_deterministic_on_repeats_batch_splits_and_the_grid_stride_loop(eng, vxo):
    """repeated calls are bit-identical; a body's result does not depend on the batch it is in; above 2^24 bodies the grid
    (capped at 65536 workgroups) strides over the batch, and every copy of a body still gets the same result"""
    vx, torch = eng
    w, vox = _world(vxo, (256, 256, 256), 32, 0.02, seed=3)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        b = R.random_bodies(np.random.default_rng(4), vox.shape, 100_000)
        db = _dev(torch, b)
        bits = lambda r: [t.view(torch.int32) for t in r]  # noqa: E731 (invalid bodies keep their NaNs: compare bits)
        first = [t.clone() for t in bits(ctx.move_boxes(db))]
        for _ in range(3):
            again = bits(ctx.move_boxes(db))
            assert all(torch.equal(x, y) for x, y in zip(first, again))
        part = bits(ctx.move_boxes(db[37:1037]))
        assert torch.equal(part[0], first[0][37:1037]) and torch.equal(part[1], first[1][37:1037])
        reps = (1 << 24) // len(b) + 2   # > 2^24 bodies
        big = db.repeat(reps, 1)
        lohi, flags = bits(ctx.move_boxes(big))
        counts, _ = ctx.overlap_boxes(big)
        c0, _ = ctx.overlap_boxes(db)
        torch.cuda.synchronize()
        assert torch.equal(lohi.view(reps, len(b), 6), first[0].unsqueeze(0).expand(reps, -1, -1))
        assert torch.equal(flags.view(reps, len(b)), first[1].unsqueeze(0).expand(reps, -1))
        assert torch.equal(counts.view(reps, len(b)), c0.unsqueeze(0).expand(reps, -1))
        wl, wf = R.move_boxes(vox, b)
        assert np.array_equal(float_bits(first[0].cpu().numpy().view(np.float32)), float_bits(wl))
        del big, lohi, flags, counts
    finally:
        ctx.close()


def test_side_stream(eng, vxo):
    vx, torch = eng
    w, vox = _world(vxo, (64, 64, 64), 8, 0.05, seed=11)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        b = R.random_bodies(np.random.default_rng(12), vox.shape, 20_000)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            db = _dev(torch, b)
            lohi, flags = ctx.move_boxes(db, stream=s.cuda_stream)
            counts, _ = ctx.overlap_boxes(db, stream=s.cuda_stream)
            out = (lohi.cpu(), flags.cpu(), counts.cpu())  # ordered on s
        s.synchronize()
        wl, wf = R.move_boxes(vox, b)
        assert np.array_equal(float_bits(out[0].numpy()), float_bits(wl)) and np.array_equal(out[1].numpy().view(np.uint32), wf)
        assert np.array_equal(out[2].numpy().view(np.uint32), R.overlap_boxes(vox, b)[0])
    finally:
        ctx.close()


def test_refusals(eng, vxo, tmp_path):
    vx, torch = eng
    L = vx.load()
    yxz = (C.c_int32 * 3)(1, 0, 2)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    host = np.zeros(64, np.float32)
    hp = host.ctypes.data
    ctx = vx.Context(0)
    try:
        assert L.vxrt_move_boxes(ctx._h, p, 1, yxz, p, None, None) == -3                     # no world
        assert L.vxrt_overlap_boxes(ctx._h, p, 1, p, None, None) == -3
        assert L.vxrt_move_boxes_host(ctx._h, hp, 1, yxz, hp, None) == -3
        assert L.vxrt_overlap_boxes_host(ctx._h, hp, 1, hp, None) == -3
        w, _ = _world(vxo, (64, 64, 64), 8, 0.05, seed=1)
        upload(ctx, w)
        for bad in ((0, 0, 1), (1, 2, 3), (-1, 0, 1), (2, 1, 2)):                            # not a permutation
            o = (C.c_int32 * 3)(*bad)
            assert L.vxrt_move_boxes(ctx._h, p, 1, o, p, None, None) == -1
            assert L.vxrt_move_boxes_host(ctx._h, hp, 1, o, hp, None) == -1
        assert L.vxrt_move_boxes(ctx._h, p, 1, None, p, None, None) == -1
        assert L.vxrt_move_boxes(ctx._h, None, 1, yxz, p, None, None) == -1                  # NULL pointers
        assert L.vxrt_move_boxes(ctx._h, p, 1, yxz, None, None, None) == -1
        assert L.vxrt_overlap_boxes(ctx._h, None, 1, p, None, None) == -1
        assert L.vxrt_overlap_boxes(ctx._h, p, 1, None, None, None) == -1
        assert L.vxrt_move_boxes_host(ctx._h, None, 1, yxz, hp, None) == -1
        assert L.vxrt_overlap_boxes_host(ctx._h, hp, 1, None, None) == -1
        assert L.vxrt_move_boxes(ctx._h, None, 0, yxz, None, None, None) == 0                # n == 0: a no-op
        assert L.vxrt_overlap_boxes(ctx._h, None, 0, None, None, None) == 0
        assert L.vxrt_move_boxes(None, p, 1, yxz, p, None, None) == -1
        with pytest.raises(ValueError):
            ctx.move_boxes(torch.zeros((4, 6), device="cuda"))
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert L.vxrt_move_boxes(ctx._h, p, 1, yxz, p, None, None) == -1                     # streamed world
        assert L.vxrt_overlap_boxes(ctx._h, p, 1, p, None, None) == -1
        assert L.vxrt_move_boxes_host(ctx._h, hp, 1, yxz, hp, None) == -1
        ctx.stream_close()
    finally:
        ctx.close()


def test_bench_world_one_million_bodies(eng):
    """1M bodies on the 8192 x 512 x 8192 bench world built on the device; 4096 of them checked against the reference on
    read_region_host of each body's swept box (no dense copy of the world)"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        dims = (8192, 512, 8192)
        b = R.random_bodies(np.random.default_rng(21), dims, 1 << 20)
        lohi, flags = ctx.move_boxes(_dev(torch, b))
        counts, oflags = ctx.overlap_boxes(_dev(torch, b))
        got = [lohi.cpu().numpy(), flags.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32),
               oflags.cpu().numpy().view(np.uint32)]
        idx = np.random.default_rng(22).choice(len(b), 4096, replace=False)
        blocked = 0
        for i in idx:
            if not R.valid(b[i])[0]:
                assert got[1][i] == R.INVALID and got[3][i] == R.INVALID and got[2][i] == 0
                assert np.array_equal(float_bits(got[0][i]), float_bits(b[i, :6]))
                continue
            o, d = R.swept_box(b[i])
            win = ctx.read_region_host(o.tolist(), d.tolist())
            wl, wf = R.move_boxes(win, b[i:i + 1], YXZ, origin=o)
            wc, _ = R.overlap_boxes(win, b[i:i + 1], origin=o)
            assert np.array_equal(float_bits(got[0][i]), float_bits(wl[0])), (i, b[i].tolist())
            assert got[1][i] == wf[0] and got[2][i] == wc[0] and got[3][i] == 0
            blocked += int(wf[0] != 0)
        assert blocked > 200
    finally:
        ctx.close()


WALK_POSES = [(64.0, 230.0, 64.0), (64.0, 190.0, 64.0), (64.0, 150.0, 64.0), (64.0, 100.0, 64.0), (90.0, 100.0, 95.0),
              (130.5, 60.25, 140.0), (131.0, 10.25, 141.5), (180.0, 12.0, 190.0), (140.0, 250.0, 140.0)]
# frame, kind, value, a, b (edit-script lines): a platform under the walk, then a hole dug through it
WALK_SCRIPT = [(1, 0, 1, (40, 170, 40), (90, 172, 90)), (4, 0, 0, (50, 150, 50), (80, 180, 80))]


def test_headless_example_walk(vxo, tmp_path):
    """examples/voxelapp_headless walk=1 with an edit script: the printed body trajectory equals the reference's moves on
    the world each frame sees (the example's world, edited up to that frame)"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    path = tmp_path / "path.txt"
    path.write_text("".join("%r %r %r -0.45 0.7 0.0\n" % p for p in WALK_POSES))
    script = tmp_path / "edits.txt"
    script.write_text("".join("%d %d %d %d %d %d %d %d %d\n" % (fr, k, v, *a, *b) for fr, k, v, a, b in WALK_SCRIPT))
    out = subprocess.run([exe, "256", "0", str(tmp_path / "w"), "64", "48", "0", str(path), "0", "1", "1", "0x0x0", str(script),
                          "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("walk frame")]
    assert len(lines) == len(WALK_POSES)
    got = np.asarray([[float.fromhex(v) for v in ln[4:7] + ln[8:11]] for ln in lines], np.float32)
    got_flags = [int(ln[12]) for ln in lines]

    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    half = np.float32([2, 6, 2])
    lo = hi = None
    want, want_flags = [], []
    for frame, pose in enumerate(WALK_POSES):
        ops = [(k, v, a, bb) for fr, k, v, a, bb in WALK_SCRIPT if fr == frame]
        if ops:
            vox = ref_edit.apply_edits(vox, ops)
        t = np.float32(pose)
        if lo is None:
            lo, hi = t - half, t + half
        d = np.clip(t - (lo + half), np.float32(-64), np.float32(64)).astype(np.float32)
        lohi, fl = R.move_boxes(vox, np.concatenate([lo, hi, d])[None], YXZ)
        lo, hi = lohi[0, :3], lohi[0, 3:]
        want.append(lohi[0])
        want_flags.append(int(fl[0]))
    assert np.array_equal(float_bits(got), float_bits(np.asarray(want))), (got, want)
    assert got_flags == want_flags
    assert any(f & 2 for f in want_flags)  # the walk does land on something
