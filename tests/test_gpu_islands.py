"""Floating-island detection on the device (include/vxrt.h, vxrt_find_islands): labels, floating bits, table and summary
equal to tests/ref_islands.py on random worlds at f = 8, 16, 32 and a wide grid, at several densities and anchor masks, on
boxes that are not multiples of the tile and boxes half outside the world; a 128^3 snake; after edits and stamps; collapse
against the oracle's brickmap; a bench-world window; truncation; determinism across calls and streams; refusals; and the
headless example's collapse line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region, vxo_edit
from tests import helpers
from tests import ref_islands as R
from tests.helpers import FACADE_POSES, assert_tables, eng, gen_dense, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = R.FACES | R.FLOOR


def _world(vxo, size, factor, density, seed):
    w = helpers.random_voxel_world(vxo, size, factor, density, seed)
    vox = np.random.default_rng(seed).random(size) < density
    return w, vox


def _labels_np(t, dims):
    return t.cpu().numpy().view(np.uint32).reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)


def _assert_islands(vx, ctx, box_vox, origin, dims, anchors, max_islands=1 << 20, labels=True, stream=None):
    """the device result against the reference computed on box_vox (the box's voxels); returns (result, reference)"""
    r = ctx.find_islands(origin, dims, anchors, labels=labels, max_islands=max_islands, stream=stream)
    want = R.fast(box_vox, origin, anchors)
    assert tuple(r.summary) == want["summary"], (origin, dims, anchors)
    assert np.array_equal(r.floating.cpu().numpy().view(np.uint32), vx.pack_region(want["floating"]))
    if labels:
        assert np.array_equal(_labels_np(r.labels, dims), want["labels"])
    assert np.array_equal(R.table_rows(r.table), want["table"][:max_islands])
    return r, want


WORLDS = [(8, (64, 64, 64)), (16, (128, 128, 128)), (32, (256, 256, 256)), (8, (8192, 64, 64))]
ANCHORS = [ALL, R.FACES, 0, R.FLOOR, R.X_LO | R.Y_HI | R.Z_LO]


@pytest.mark.parametrize("factor,size", WORLDS)
@pytest.mark.parametrize("density", [0.05, 0.2, 0.31])
def test_islands_equal_the_reference(eng, vxo, factor, size, density):
    vx, torch = eng
    w, vox = _world(vxo, size, factor, density, seed=factor + size[0] + int(density * 100))
    rng = np.random.default_rng(factor * 7 + size[0])
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        boxes = [((0, 0, 0), tuple(min(s, 160) for s in size)), ((-40, -30, -50), (97, 70, 101)),
                 ((size[0] - 50, 3, size[2] - 20), (100, 61, 45)), ((5, 7, 9), (1, 33, 17)), ((2, 1, 0), (200, 1, 3))]
        for _ in range(3):
            d = tuple(int(rng.integers(1, 120)) for _ in range(3))
            o = tuple(int(rng.integers(-20, s)) for s in size)
            boxes.append((o, d))
        for k, (o, d) in enumerate(boxes):
            _assert_islands(vx, ctx, ref_region.read_region(vox, o, d), o, d, ANCHORS[k % len(ANCHORS)], labels=k % 2 == 0)
        # the host form gives the same
        o, d = boxes[1]
        h = ctx.find_islands_host(o, d, ALL, labels=True, max_islands=1 << 20)
        want = R.fast(ref_region.read_region(vox, o, d), o, ALL)
        assert tuple(h.summary) == want["summary"] and np.array_equal(h.floating, want["floating"])
        assert np.array_equal(h.labels, want["labels"]) and np.array_equal(R.table_rows(h.table), want["table"])
    finally:
        ctx.close()


def test_spiral_snake_spanning_a_128_box(eng, vxo):
    vx, torch = eng
    vox = np.zeros((128, 128, 128), bool)
    vox[1:127, 1:127, 1:127] = R.snake((126, 126, 126))
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        r, want = _assert_islands(vx, ctx, vox, (0, 0, 0), (128, 128, 128), R.FACES)
        assert r.summary == (1, 1, int(vox.sum())) and r.table[0]["id"] == 1 + 1 + 128 * (1 + 128)
        cut = vox.copy()
        cut[64, 1, 1] = False
        ctx.edit_voxels([vx.EditBox((64, 1, 1), (64, 1, 1), 0)])
        r, _ = _assert_islands(vx, ctx, cut, (0, 0, 0), (128, 128, 128), 0)
        assert r.summary[0] == 2
    finally:
        ctx.close()


def test_results_follow_edits_and_stamps(eng, vxo):
    vx, torch = eng
    w, vox = _world(vxo, (128, 128, 128), 16, 0.25, seed=11)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        rng = np.random.default_rng(12)
        ops = [(0, 0, (0, 40, 0), (127, 44, 127)), (1, 1, (64, 60, 64), (15, 0, 0)), (0, 0, (10, 0, 10), (30, 127, 30))]
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        stamps = [((20, 60, 20), rng.random((50, 10, 70)) < 0.5, vx.STAMP_UNION),
                  ((-5, 30, 50), np.ones((60, 20, 40), bool), vx.STAMP_SUBTRACT)]
        ctx.edit_stamps([vx.Stamp(o, m, mode) for o, m, mode in stamps])
        for o, d, anchors in [((0, 0, 0), (128, 128, 128), ALL), ((10, 30, 5), (90, 40, 100), R.FACES), ((-3, 50, 60), (77, 33, 80), 0)]:
            box = ctx.read_region_host(o, d)  # the reference runs on the device's own voxels
            _assert_islands(vx, ctx, box, o, d, anchors)
        vox = ref_region.apply_stamps(ref_edit.apply_edits(vox, ops), stamps)
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (128, 128, 128)), vox)
    finally:
        ctx.close()


def test_collapse_leaves_the_oracle_world_and_no_islands(eng, vxo):
    vx, torch = eng
    X = Y = Z = 128
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    vox = vxo_edit.voxels_from_dense(dense, X, Y, Z)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_dense(dense, X, Y, Z, 16))
        # an overhang on a stem, then a dig through the stem and a pocket of loose voxels under the terrain surface
        ops = [(0, 1, (40, 100, 40), (60, 102, 60)), (0, 1, (50, 60, 50), (51, 99, 51)), (0, 0, (45, 80, 45), (55, 82, 55)),
               (1, 0, (90, 40, 90), (12, 0, 0)), (0, 1, (88, 38, 88), (92, 42, 92))]
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        vox = ref_edit.apply_edits(vox, ops)
        o, d = (30, 30, 30), (80, 90, 80)
        want = R.fast(ref_region.read_region(vox, o, d), o, ALL)
        assert want["summary"][1] >= 2
        isl, st = ctx.collapse_islands(o, d)
        assert tuple(isl.summary) == want["summary"]
        assert np.array_equal(R.table_rows(isl.table), want["table"])
        assert st.bricks_touched > 0
        after = ref_region.apply_stamps(vox, [(o, want["floating"], vx.STAMP_SUBTRACT)])
        assert_tables(ctx, vxo.World.from_dense(vxo.dense_from_voxels(after), X, Y, Z, 16))
        again = ctx.find_islands(o, d)
        assert again.summary.islands == 0 and again.summary.island_voxels == 0
        assert again.summary.components == want["summary"][0] - want["summary"][1]
    finally:
        ctx.close()


def test_bench_world_window(eng):
    """a 256 x 512 x 256 window (2^25 voxels) of the bench world against the reference on read_region_host"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        for o, d, anchors in [((4000, 0, 3000), (256, 512, 256), ALL), ((100, 100, 7000), (300, 300, 300), R.FACES)]:
            box = ctx.read_region_host(o, d)
            r, want = _assert_islands(vx, ctx, box, o, d, anchors, labels=True)
            assert want["summary"][0] > 0
    finally:
        ctx.close()


def test_truncated_table_keeps_the_true_count(eng, vxo):
    vx, torch = eng
    w, vox = _world(vxo, (64, 64, 64), 8, 0.2, seed=3)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        for m in (0, 1, 5):
            r, want = _assert_islands(vx, ctx, vox, (0, 0, 0), (64, 64, 64), ALL, max_islands=m, labels=False)
            assert want["summary"][1] > 5 and len(r.table) == m
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams(eng, vxo):
    vx, torch = eng
    w, vox = _world(vxo, (256, 256, 256), 32, 0.31, seed=5)
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        o, d = (-5, 3, 7), (250, 240, 230)
        first = ctx.find_islands(o, d, ALL, labels=True)
        side = torch.cuda.Stream()
        for k in range(3):
            s = side.cuda_stream if k == 2 else None
            r = ctx.find_islands(o, d, ALL, labels=True, stream=s)
            assert torch.equal(r.floating, first.floating) and torch.equal(r.labels, first.labels)
            assert r.table.tobytes() == first.table.tobytes() and r.summary == first.summary
        want = R.fast(ref_region.read_region(vox, o, d), o, ALL)
        assert tuple(first.summary) == want["summary"]
    finally:
        ctx.close()


def test_refusals(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        buf = torch.zeros(1 << 20, dtype=torch.int32, device="cuda")
        p = buf.data_ptr()            # workspace
        fl, sp = p + (1 << 21), p + (1 << 21) + (1 << 20)  # floating words, summary: apart from the workspace
        o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
        host = np.zeros(1 << 12, np.uint32)
        sm = np.zeros(3, np.uint32)
        assert L.vxrt_find_islands(h, o3, d3, 0, p, fl, None, None, 0, sp, None) == -3        # no world
        assert L.vxrt_find_islands_host(h, o3, d3, 0, host.ctypes.data, None, None, 0, sm.ctypes.data) == -3
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        for bad in [(0, 8, 8), (8, -1, 8), (1024, 1024, 257)]:                              # bad dims
            assert L.vxrt_find_islands(h, o3, (C.c_int32 * 3)(*bad), 0, p, fl, None, None, 0, sp, None) == -1
        assert L.vxrt_find_islands(h, (C.c_int32 * 3)(2 ** 31 - 4, 0, 0), d3, 0, p, fl, None, None, 0, sp, None) == -1
        for bad in (0x80, 0x100, 0xFFFFFFFF):                                                   # anchor bits
            assert L.vxrt_find_islands(h, o3, d3, bad, p, fl, None, None, 0, sp, None) == -1
        assert L.vxrt_find_islands(h, o3, d3, 0x7F, p, fl, None, None, 0, sp, None) == 0
        torch.cuda.synchronize()
        for args in [(None, d3, p, fl, sp), (o3, None, p, fl, sp), (o3, d3, None, fl, sp), (o3, d3, p, None, sp), (o3, d3, p, fl, None)]:
            a, b, wk, fl, s = args
            assert L.vxrt_find_islands(h, a, b, 0, wk, fl, None, None, 0, s, None) == -1
        assert L.vxrt_find_islands_host(h, o3, d3, 0, None, None, None, 0, sm.ctypes.data) == -1
        assert L.vxrt_find_islands_host(h, o3, d3, 0, host.ctypes.data, None, None, 0, None) == -1
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert L.vxrt_find_islands(h, o3, d3, 0, p, fl, None, None, 0, sp, None) == -1          # streamed world
        assert L.vxrt_find_islands_host(h, o3, d3, 0, host.ctypes.data, None, None, 0, sm.ctypes.data) == -1
        ctx.stream_close()
    finally:
        ctx.close()


def test_headless_example_collapse_script(vxo, tmp_path):
    """examples/voxelapp_headless: build an overhang on a stem (kind 0), dig through the stem, collapse (kind 4): the printed
    summary equals the reference's, and the last frame equals the oracle's frame of the world without the island"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    W_, H_ = 160, 96
    edge = 256
    script = [(0, 0, 1, (60, 200, 60), (110, 206, 110)), (0, 0, 1, (84, 150, 84), (86, 199, 86)),
              (1, 0, 0, (80, 180, 80), (90, 184, 90)), (1, 4, 0, (50, 140, 50), (70, 80, 70))]
    path = tmp_path / "path.txt"
    path.write_text("".join("%r %r %r %r %r %r\n" % (*p, *e) for p, e in FACADE_POSES[:2]))
    sf = tmp_path / "edits.txt"
    sf.write_text("".join("%d %d %d %d %d %d %d %d %d\n" % (fr, k, v, *a, *b) for fr, k, v, a, b in script))
    prefix = str(tmp_path / "co")
    out = subprocess.run([exe, str(edge), "0", prefix, str(W_), str(H_), "1", str(path), "1", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    vox = ref_edit.apply_edits(vox, [(k, v, a, b) for fr, k, v, a, b in script if k != 4])
    o, d = (50, 140, 50), (70, 80, 70)
    want = R.fast(ref_region.read_region(vox, o, d), o, ALL)
    assert want["summary"][1] >= 1 and want["summary"][2] >= 51 * 7 * 51
    line = [s for s in out.stdout.splitlines() if s.startswith("collapse before frame 1:")]
    assert len(line) == 1 and line[0].startswith("collapse before frame 1: %d components, %d islands, %d island voxels,"
                                                  % want["summary"]), out.stdout
    vox = ref_region.apply_stamps(vox, [(o, want["floating"], vx_subtract())])
    w = vxo.World.from_dense(vxo.dense_from_voxels(vox), edge, edge, edge, 32)
    pos, euler = FACADE_POSES[1]
    f, u, r = vxo.get_directions(euler)
    p0 = FACADE_POSES[0]
    fb0 = vxo.World.from_dense(vxo.dense_from_voxels(ref_edit.apply_edits(
        vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge),
        [(k, v, a, b) for fr, k, v, a, b in script if fr == 0])), edge, edge, edge, 32)
    f0, u0, r0 = vxo.get_directions(p0[1])
    prm0 = vxo.make_params(W_, H_, tuple(np.float32(v) for v in p0[0]), f0, u0, r0, frame_number=0, mode=vxo.MODE_SHADED,
                           checkerboard=1, shadow=1, bounce_samples=1)
    fb = fb0.render(prm0, fb=np.full((H_, W_, 4), 255, np.uint8), nthreads=16)["fb"]
    prm = vxo.make_params(W_, H_, tuple(np.float32(v) for v in pos), f, u, r, frame_number=1, mode=vxo.MODE_SHADED,
                          checkerboard=1, shadow=1, bounce_samples=1)
    fb = w.render(prm, fb=fb.copy(), nthreads=16)["fb"]
    head = b"P6\n%d %d\n255\n" % (W_, H_)
    raw = open("%s_%04d.ppm" % (prefix, 1), "rb").read()
    rgb = np.frombuffer(raw[len(head):], np.uint8).reshape(H_, W_, 3)
    assert np.array_equal(rgb, fb[:, :, [2, 1, 0]])


def vx_subtract():
    import voxelengine_amd as vx
    return vx.STAMP_SUBTRACT
