"""Voxel piece queries on the device (include/vxrt.h, vxrt_place_pieces) and the falling islands built on them: every result
bit-equal to the restatements of tests/ref_place.py -- on random worlds at f = 8, 16 and 32, at every x alignment, at the
distance limit, with pieces of many workgroups, against the box queries, after edits and stamps, on side streams, in split
batches, with guard words behind the results, through every refusal and on a window of the bench world.

World sizes: the world builder of the tests takes whole tiles of 8 x 8 x 8 coarse cells, so the worlds are the smallest such
that hold each case (64^3 at f = 8, 128^3 at f = 16, 256^3 at f = 32, 64 x 4160 x 64 for the distance limit); the big pieces
hang out of their world, which reads as empty there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, vxo_edit
from tests import place_cases as PC
from tests import ref_islands
from tests import ref_place as R
from tests.helpers import FACADE_POSES, eng, gen_dense, upload
from tests.test_place_host import classes, random_pieces, random_placements, random_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx(vx, vxo, vox, factor):
    ctx = vx.Context(0)
    upload(ctx, vxo.World.from_voxels(vox, factor))
    return ctx


def _dev(torch, a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _place(vx, torch, ctx, pieces, pl, stream=None):
    """place_pieces of bool grids / Piece objects; the (n, 4) uint32 words of the results"""
    ps = [p if isinstance(p, vx.Piece) else vx.Piece(p) for p in pieces]
    out = ctx.place_pieces(ps, _dev(torch, np.asarray(pl).reshape(-1, 6)), stream=stream)
    if stream is None:
        torch.cuda.synchronize()
    return out


def _assert_place(vx, torch, ctx, vox, pieces, pl, how=R.place_clearance, dev_pieces=None):
    got = _place(vx, torch, ctx, dev_pieces or pieces, pl).cpu().numpy().view(np.uint32)
    want = R.place(vox, pieces, pl, how)
    bad = np.flatnonzero((got != R.pack_results(want)).any(1))
    assert len(bad) == 0, (len(bad), np.asarray(pl).reshape(-1, 6)[bad[:3]].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())
    return want


@pytest.mark.parametrize("factor,size", [(8, (64, 64, 64)), (16, (128, 128, 128)), (32, (256, 256, 256))])
def test_random_worlds(eng, vxo, factor, size):
    """4000 placements of ten pieces -- one voxel, sparse, 31 / 32 / 33 / 64 / 65 wide, many rows, empty, padding bits set --
    origins from -8 to the world's far side, every axis, dist -12 .. 12: each class of result at least a tenth"""
    vx, torch = eng
    rng = np.random.default_rng(factor)
    vox = random_world(rng, size)
    pieces = random_pieces(rng)
    ctx = _ctx(vx, vxo, vox, factor)
    try:
        dev = [vx.Piece(p) for p in pieces]
        dev[-1] = vx.Piece(_dev(torch, PC.padded_words(pieces[-1]).view(np.int32)), pieces[-1].shape)
        pl = random_placements(rng, size, 4000, len(pieces))
        want = _assert_place(vx, torch, ctx, vox, pieces, pl, dev_pieces=dev)
        shares = classes(want)
        print("class shares", shares)
        assert min(shares) >= 0.1, shares
        # the host call gives the device path's results
        hp = [vx.Piece(p) for p in pieces]
        got = ctx.place_pieces_host(hp, pl[:500])
        assert np.array_equal(got.view(np.uint32).reshape(-1, 4), R.pack_results(want[:500]))
        got = ctx.place_pieces_host([vx.Piece(PC.cube())], [vx.Placement(0, (3, 40, 3), 1, -5)])
        assert got.view(np.uint32).reshape(-1, 4).tolist() == R.pack_results(R.place(vox, [PC.cube()], [[0, 3, 40, 3, 1, -5]])).tolist()
    finally:
        ctx.close()


def test_every_x_alignment(eng, vxo):
    """a 33 x 2 x 2 piece at every origin x from -40 to 72 of a 64-wide world at f = 8, swept 40 both ways along x: every
    residue mod 32, negative origins, brick borders and the end of the world"""
    vx, torch = eng
    rng = np.random.default_rng(11)
    vox = random_world(rng, (64, 64, 64), 0.02)
    piece = rng.random((33, 2, 2)) < 0.5
    ctx = _ctx(vx, vxo, vox, 8)
    try:
        pl = [[0, x, y, z, 0, d] for x in range(-40, 73) for d in (-40, 40) for y, z in ((5, 9), (20, 33), (40, 62))]
        want = _assert_place(vx, torch, ctx, vox, [piece], pl, how=R.place_shift)
        assert np.count_nonzero(want[:, 3]) > 50 and np.count_nonzero(want[:, 3] == 0) > 50
    finally:
        ctx.close()


def test_the_distance_limit(eng, vxo):
    vx, torch = eng
    vox = np.zeros((64, 4160, 64), bool)
    vox[3, 4100, 3] = True
    one = np.ones((1, 1, 1), bool)
    ctx = _ctx(vx, vxo, vox, 8)
    try:
        pl = [[0, 3, 4, 3, 1, 4096], [0, 3, 4, 3, 1, 4095], [0, 3, 4, 3, 1, -4096], [0, 3, 4, 3, 1, 4097], [0, 3, 4, 3, 1, -4097]]
        want = _assert_place(vx, torch, ctx, vox, [one], pl)
        assert want.tolist() == [[0, 4095, 1, 1], [0, 4095, 0, 0], [0, -4096, 0, 0], [0, 0, 0, 2], [0, 0, 0, 2]]
    finally:
        ctx.close()


def test_big_pieces_over_many_workgroups(eng, vxo):
    """a 256^3 piece (1024 tasks) and a 1024 x 128 x 128 one (2^24 voxels): a fit, a drop onto the floor and a sweep along x;
    overlap and contact are sums over all tasks, the travel a minimum over them"""
    vx, torch = eng
    rng = np.random.default_rng(12)
    vox = np.zeros((256, 256, 256), bool)
    vox[:, :32, :] = True  # a floor
    vox[230:, 32:200, :40] = rng.random((26, 168, 40), dtype=np.float32) < 0.02  # and something to run into along x
    a = rng.random((256, 256, 256), dtype=np.float32) < 0.001
    a[255, 255, 255] = True
    b = rng.random((1024, 128, 128), dtype=np.float32) < 0.001
    ctx = _ctx(vx, vxo, vox, 32)
    try:
        for piece, pl in ((a, [[0, -20, 20, 10, 1, 0], [0, -40, 45, 10, 1, -40], [0, -40, 40, 0, 0, 60]]),
                          (b, [[0, -300, 25, 60, 2, 0], [0, -300, 45, 60, 1, -40], [0, -810, 40, -100, 0, 50]])):
            want = _assert_place(vx, torch, ctx, vox, [piece], pl, how=R.place_shift)
            assert want[0, 0] > 100 and want[1, 3] == R.BLOCKED and want[1, 1] < -5 and want[2, 3] == R.BLOCKED, want
    finally:
        ctx.close()


def test_agreement_with_the_box_queries(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(13)
    size = (128, 128, 128)
    vox = random_world(rng, size, 0.001)
    shapes = [(1, 2, 1), (3, 3, 3), (12, 5, 7), (33, 2, 4), (64, 3, 2), (2, 64, 2)]
    pieces = [np.ones(s, bool) for s in shapes]
    ctx = _ctx(vx, vxo, vox, 16)
    try:
        pl = random_placements(rng, size, 6000, len(pieces), dmax=64)
        want = _assert_place(vx, torch, ctx, vox, pieces, pl)
        lo = pl[:, 1:4].astype(np.float32)
        hi = lo + np.asarray(shapes, np.float32)[pl[:, 0]]
        delta = np.zeros((len(pl), 3), np.float32)
        delta[np.arange(len(pl)), pl[:, 4]] = pl[:, 5]
        bodies = torch.from_numpy(np.concatenate([lo, hi, delta], 1)).cuda()
        counts, _ = ctx.overlap_boxes(bodies)
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), want[:, 0].astype(np.uint32))
        lohi, flags = ctx.move_boxes(bodies)
        free = want[:, 0] == 0
        assert np.count_nonzero(free) >= 0.3 * len(pl)
        moved = lohi.cpu().numpy()[free, :3] - lo[free]
        assert np.array_equal(moved[np.arange(len(moved)), pl[free, 4]], want[free, 1].astype(np.float32))
        blocked = flags.cpu().numpy()[free] == (1 << pl[free, 4])
        assert np.array_equal(blocked, want[free, 3] == R.BLOCKED) and np.count_nonzero(blocked) > 200
    finally:
        ctx.close()


def test_after_edits_and_stamps(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(14)
    vox = random_world(rng, (64, 64, 64), 0.05)
    ctx = _ctx(vx, vxo, vox, 8)
    try:
        o, d = (5, 3, 7), (45, 20, 30)
        words = ctx.read_region(o, d)
        piece = vx.Piece(words, d)
        grid = vox[5:50, 3:23, 7:37]
        res = _place(vx, torch, ctx, [piece], [[0, *o, 1, 0]]).cpu().numpy()
        assert res[0].tolist() == [int(grid.sum()), 0, 0, 0] and grid.sum() > 1000
        ctx.edit_stamps([vx.Stamp(o, words, vx.STAMP_SUBTRACT, d)])
        vox[5:50, 3:23, 7:37] = False
        assert _place(vx, torch, ctx, [piece], [[0, *o, 1, 0]]).cpu().numpy()[0].tolist() == [0, 0, 0, 0]
        # a cube above the hole falls through it to the world's floor, until a box edit closes the path, and again when it opens
        cube = PC.cube(3)
        pl = [[0, 20, 24, 20, 1, -24], [0, 20, 24, 20, 0, 30]]
        vox[18:26, 23:30, 18:26] = False
        ctx.edit_voxels([vx.EditBox((18, 23, 18), (25, 29, 25), 0)])
        open_ = _assert_place(vx, torch, ctx, vox, [cube], pl)
        vox[:, 10, :] = True
        ctx.edit_voxels([vx.EditBox((0, 10, 0), (63, 10, 63), 1)])
        shut = _assert_place(vx, torch, ctx, vox, [cube], pl)
        assert shut[0].tolist() == [0, -13, 9, 1] and open_[0, 1] < -13
        vox[:, 10, :] = False
        ctx.edit_voxels([vx.EditBox((0, 10, 0), (63, 10, 63), 0)])
        assert np.array_equal(_assert_place(vx, torch, ctx, vox, [cube], pl), open_)
    finally:
        ctx.close()


def _assert_drop(vx, ctx, vox, o, d, anchors=ref_islands.FACES | ref_islands.FLOOR):
    want_world, want_rows = R.drop_islands(vox, o, d, anchors)
    rows = ctx.drop_islands(o, d, anchors)
    got = np.column_stack([rows["id"], rows["voxels"], rows["travel"], rows["contact"]]).astype(np.int64).reshape(-1, 4)
    assert np.array_equal(got, want_rows), (got[:5], want_rows[:5])
    assert np.array_equal(ctx.read_region_host((0, 0, 0), vox.shape), want_world)
    return want_world, want_rows


@pytest.mark.parametrize("case", PC.DROP_CASES, ids=[c[0] for c in PC.DROP_CASES])
def test_falling_island_cases(eng, vxo, case):
    vx, torch = eng
    _, small, o, d, want_rows = case
    vox = np.zeros((64, 64, 64), bool)
    vox[:16, :16, :16] = small
    ctx = _ctx(vx, vxo, vox, 8)
    try:
        after, rows = _assert_drop(vx, ctx, vox, o, d)
        assert rows.tolist() == [list(r) for r in want_rows] and after.sum() == vox.sum()
    finally:
        ctx.close()


def test_falling_slab_and_refusal(eng, vxo):
    """a box edit cuts a slab loose from a random world: it lands with the debris around it; a table too short refuses with
    the world unchanged"""
    vx, torch = eng
    rng = np.random.default_rng(15)
    vox = random_world(rng, (64, 64, 64), 0.004)
    vox[10:40, 40:44, 12:50] = True   # a slab ...
    vox[24:26, 16:40, 30:32] = True   # ... on a stem
    ctx = _ctx(vx, vxo, vox, 8)
    try:
        ctx.edit_voxels([vx.EditBox((20, 30, 26), (30, 33, 36), 0)])  # through the stem
        vox[20:31, 30:34, 26:37] = False
        o, d = (2, 14, 2), (60, 48, 60)
        with pytest.raises(ValueError):
            ctx.drop_islands(o, d, max_islands=1)
        assert np.array_equal(ctx.read_region_host((0, 0, 0), vox.shape), vox)
        after, rows = _assert_drop(vx, ctx, vox, o, d)
        # (an island that lands where a later one still hung merges with it when that one falls: voxels may only be lost so)
        assert len(rows) > 5 and rows[:, 1].max() >= 30 * 4 * 38 and rows[:, 2].min() < 0 and after.sum() <= vox.sum()
    finally:
        ctx.close()


def test_headless_example_drop_script(vxo, tmp_path):
    """examples/voxelapp_headless: build an overhang on a stem (kind 0), dig through the stem, drop (kind 11): the printed
    lines equal the restatement's rows"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    script = [(0, 0, 1, (60, 200, 60), (110, 206, 110)), (0, 0, 1, (84, 150, 84), (86, 199, 86)),
              (1, 0, 0, (80, 180, 80), (90, 184, 90)), (1, 11, 0, (50, 140, 50), (70, 80, 70))]
    path = tmp_path / "path.txt"
    path.write_text("".join("%r %r %r %r %r %r\n" % (*p, *e) for p, e in FACADE_POSES[:2]))
    sf = tmp_path / "edits.txt"
    sf.write_text("".join("%d %d %d %d %d %d %d %d %d\n" % (fr, k, v, *a, *b) for fr, k, v, a, b in script))
    out = subprocess.run([exe, str(edge), "0", str(tmp_path / "dr"), "160", "96", "1", str(path), "1", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    vox = ref_edit.apply_edits(vox, [(k, v, a, b) for fr, k, v, a, b in script if k != 11])
    _, rows = R.drop_islands(vox, (50, 140, 50), (70, 80, 70))
    assert len(rows) >= 1 and rows[:, 1].max() >= 51 * 7 * 51 and rows[:, 2].min() < 0
    want = "drop before frame 1: %d islands, %d island voxels, %d moved, max_fall %d, sum_contact %d" % (
        len(rows), rows[:, 1].sum(), np.count_nonzero(rows[:, 2]), max(0, -rows[:, 2].min()), rows[:, 3].sum())
    h = 0xcbf29ce484222325
    for byte in R.pack_results(rows).tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    lines = out.stdout.splitlines()
    assert want in lines, [s for s in lines if s.startswith("drop")]
    assert "drop hash frame 1 rows %016x" % h in lines, [s for s in lines if s.startswith("drop")]


def test_determinism_batches_and_streams(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(16)
    vox = random_world(rng, (64, 64, 64))
    pieces = [vx.Piece(p) for p in random_pieces(rng)]
    ctx = _ctx(vx, vxo, vox, 8)
    try:
        pl = random_placements(rng, (64, 64, 64), 3000, len(pieces))
        first = _place(vx, torch, ctx, pieces, pl)
        for _ in range(2):
            assert torch.equal(_place(vx, torch, ctx, pieces, pl), first)
        halves = torch.cat([_place(vx, torch, ctx, pieces, pl[:1500]), _place(vx, torch, ctx, pieces, pl[1500:])])
        assert torch.equal(halves, first)
        # a batch of the small pieces alone has another launch shape and the same results
        small = np.flatnonzero(np.isin(pl[:, 0], (0, 2, 3)))
        assert torch.equal(_place(vx, torch, ctx, pieces[:4], pl[small]), first[torch.from_numpy(small).cuda()])
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = _place(vx, torch, ctx, pieces, pl, stream=side.cuda_stream)
        side.synchronize()
        assert torch.equal(got, first)
    finally:
        ctx.close()


def test_host_placements_on_a_side_stream_and_pieces_dropped_after_the_call(eng, vxo):
    """place_pieces with a list of Placement copies it on torch's current stream and launches on ``stream``; every reference
    to the pieces' device words is dropped as soon as it returns, and memory of their sizes is handed out and overwritten on
    torch's current stream while the side stream may still run.  The results equal the default stream's: nothing but the
    call itself keeps the launch's inputs alive (64^3 is the smallest world of factor 8: 8 coarse cells per axis)"""
    vx, torch = eng
    rng = np.random.default_rng(23)
    vox = random_world(rng, (64, 64, 64))
    grids = random_pieces(rng)
    ctx = _ctx(vx, vxo, vox, 8)
    try:
        pl = random_placements(rng, (64, 64, 64), 500, len(grids))
        first = _place(vx, torch, ctx, grids, pl)
        rows = [vx.Placement(int(r[0]), (int(r[1]), int(r[2]), int(r[3])), int(r[4]), int(r[5])) for r in pl]
        pieces = [vx.Piece(_dev(torch, vx.pack_region(g).view(np.int32)), g.shape) for g in grids]
        sizes = [p.bits.numel() for p in pieces] + [pl.size]
        side = torch.cuda.Stream()
        got = ctx.place_pieces(pieces, rows, stream=side.cuda_stream)
        del pieces
        junk = [torch.full((k,), -1, dtype=torch.int32, device="cuda") for k in sizes]
        side.synchronize()
        assert torch.equal(got, first)
        del junk
    finally:
        ctx.close()


def test_memory_and_refusals(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        bits = torch.ones(64, dtype=torch.int32, device="cuda")
        n = 100
        pl = np.tile(np.asarray([0, 3, 40, 3, 1, -5], np.int32), (n, 1))
        d_pl = _dev(torch, pl)
        res = torch.full((n * 4 + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")

        def piece(ptr=bits.data_ptr(), dims=(2, 2, 2), reserved=0):
            p = vx.PieceDesc()
            p.d_bits, p.dims, p.reserved = ptr, (C.c_int32 * 3)(*dims), reserved
            return (vx.PieceDesc * 1)(p)

        def call(pieces=None, n_pieces=1, pls=d_pl.data_ptr(), count=n, out=res.data_ptr()):
            return L.vxrt_place_pieces(h, piece() if pieces is None else pieces, n_pieces, pls, count, out, None)

        host_pl, host_res, host_bits = pl.copy(), np.zeros((n, 4), np.uint32), np.ones(64, np.uint32)
        # with no world resident: the argument checks come first, then n == 0, then the NULL checks, then the world
        assert L.vxrt_place_pieces(None, piece(), 1, d_pl.data_ptr(), n, res.data_ptr(), None) == -1
        for bad in (0, 65):
            assert call(n_pieces=bad) == -1
        assert L.vxrt_place_pieces(h, None, 1, d_pl.data_ptr(), n, res.data_ptr(), None) == -1
        for bad in (piece(ptr=None), piece(reserved=1), piece(dims=(0, 2, 2)), piece(dims=(2, 1025, 2)), piece(dims=(2, 2, -1)),
                    piece(dims=(1024, 1024, 17))):
            assert call(pieces=bad) == -1
            assert call(pieces=bad, count=0) == -1  # before the no-op
        assert call(count=0) == 0 and call(count=0, pls=None, out=None) == 0
        assert call(pls=None) == -1 and call(out=None) == -1
        assert call() == -3  # no world
        assert L.vxrt_place_pieces_host(h, piece(ptr=host_bits.ctypes.data), 1, host_pl.ctypes.data, n, host_res.ctypes.data) == -3
        assert L.vxrt_place_pieces_host(h, piece(ptr=host_bits.ctypes.data), 1, None, n, host_res.ctypes.data) == -1
        assert call(pieces=piece(dims=(1024, 1024, 16))) == -3  # 2^24 voxels is within the limits

        big = np.zeros((64, 64, 64), bool)
        big[:, :32, :] = True
        upload(ctx, vxo.World.from_voxels(big, 8))
        # invalid placements are flagged, their neighbours' results intact, and nothing is written behind the results
        pl[7] = [1, 3, 40, 3, 1, -5]
        pl[8] = [0, 3, 40, 3, 3, -5]
        pl[50] = [0, 3, 40, 3, 1, 4097]
        pl[99] = [0, (1 << 30) + 1, 40, 3, 1, -5]
        d_pl = _dev(torch, pl)
        assert call(pls=d_pl.data_ptr()) == 0
        torch.cuda.synchronize()
        got = res.cpu().numpy()
        assert np.all(got[n * 4:] == 0x5A5A5A5A)
        want = R.place(big, [PC.cube()], pl)
        assert np.array_equal(got[: n * 4].view(np.uint32).reshape(-1, 4), R.pack_results(want))
        assert want[0].tolist() == [0, -5, 0, 0] and [i for i in range(n) if want[i, 3] == R.INVALID] == [7, 8, 50, 99]
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert call(pls=d_pl.data_ptr()) == -1  # a streamed world
        assert L.vxrt_place_pieces_host(h, piece(ptr=host_bits.ctypes.data), 1, host_pl.ctypes.data, n, host_res.ctypes.data) == -1
        ctx.stream_close()
    finally:
        ctx.close()


def test_bench_world_window(eng):
    """4096 placements of three pieces inside a 256 x 128 x 256 window of the bench world, piece and sweep inside the window,
    against the restatement on read_region_host of the window"""
    vx, torch = eng
    rng = np.random.default_rng(17)
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        fill = ctx.read_region_host((4000, 0, 3000), (64, 512, 64)).mean(axis=(0, 2))  # solid share per y: the surface is
        surface = int(np.argmax(fill < 0.5))                                            # where it falls below a half
        o, d = (4000, min(max(surface - 64, 0), 384), 3000), (256, 128, 256)
        box = ctx.read_region_host(o, d)
        pieces = [np.ones((1, 2, 1), bool), rng.random((9, 5, 7)) < 0.3, rng.random((33, 4, 3)) < 0.5]
        n = 4096
        pl = np.zeros((n, 6), np.int32)
        pl[:, 0] = rng.integers(0, 3, n)
        pl[:, 4] = rng.integers(0, 3, n)
        pl[:, 5] = rng.integers(-12, 13, n)
        for k in range(3):
            pl[:, 1 + k] = rng.integers(12, d[k] - 33 - 12, n)  # piece plus sweep inside the window
        want = R.place(box, pieces, pl)
        pl[:, 1:4] += np.asarray(o, np.int32)
        got = _place(vx, torch, ctx, pieces, pl).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, R.pack_results(want))
        assert np.count_nonzero(want[:, 3]) > 400 and np.count_nonzero(want[:, 0] == 0) > 400
    finally:
        ctx.close()
