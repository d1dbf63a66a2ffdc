"""Voxel editing on the device (include/vxrt.h, vxrt_edit_voxels; an extension: the reference lists "Fully modifiable
terrain" as to do, README.md:16).  After every edit call the resident tables must be what the oracle's brickmap builder
makes of the oracle-edited dense grid (coarse bits, extents, brick contents; slot numbers excepted), and frames and batches
must equal the oracle's on that world, byte for byte."""
import numpy as np
import pytest

from oracle import vxo_edit
from tests import helpers
from tests.helpers import (FACADE_POSES, assert_batch, assert_frames, assert_tables, eng, gen_dense, new_ctx, oracle_frame,
                           random_ops, upload)

pytestmark = pytest.mark.gpu
BOX, SPHERE = 0, 1
W, H = 64, 48

WORLDS = [  # (factor, X, Y, Z, how the world is made)
    (8, 64, 64, 64, "upload"),
    (16, 128, 128, 128, "device"),
    (32, 256, 256, 256, "upload"),
    (8, 8192, 64, 64, "upload"),    # a wide grid: 1024 x 8 x 8 cells, a 4 MiB dense oracle grid
]


@pytest.mark.parametrize("factor,X,Y,Z,how", WORLDS)
def test_random_edit_sequences_equal_the_oracle(eng, vxo, factor, X, Y, Z, how):
    vx, torch = eng
    rng = np.random.default_rng(factor * 7 + X)
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx, twin = new_ctx(vx), new_ctx(vx)
    try:
        for c in (ctx, twin):
            if how == "device":
                c.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
            else:
                upload(c, vxo.World.from_dense(dense, X, Y, Z, factor))
        assert_tables(ctx, vxo.World.from_dense(dense, X, Y, Z, factor))
        created = freed = 0
        for call in range(20):
            ops = random_ops(rng, (X, Y, Z), int(rng.integers(1, 65)), max(min(X, Y, Z) // 2, 4))
            st = ctx.edit_voxels(ops)
            st2 = twin.edit_voxels([vx.EditBox(a, b, v) if k == BOX else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
            dense = vxo_edit.apply_edits(dense, X, Y, Z, ops)
            w = vxo.World.from_dense(dense, X, Y, Z, factor)
            d = assert_tables(ctx, w)
            assert st.bricks_live == int((w.brick_slot != 0xFFFFFFFF).sum()) and st.pool_slots == d["pool"].size // (factor ** 3 // 32)
            assert st.pool_capacity >= st.pool_slots
            created, freed = created + st.bricks_created, freed + st.bricks_freed
            # determinism: the same calls on a second context give byte-identical downloads, pool included
            d2 = twin.download_world()
            assert all(np.array_equal(d[k], d2[k]) for k in ("coarse_bits", "brick_slot", "bounds", "pool"))
            assert (st.bricks_created, st.bricks_freed, st.pool_slots) == (st2.bricks_created, st2.bricks_freed, st2.pool_slots)
            full = call % 5 == 4
            assert_frames(vx, ctx, torch, vxo, w, cams="ABCD" if full else "A", variants=(4, 1) if full else (4,))
            if full:
                assert_batch(ctx, w, seed=call)
        assert created > 0 and freed > 0
    finally:
        ctx.close()
        twin.close()


def test_freed_slots_are_reused_and_growth_follows_capacity(eng, vxo):
    vx, torch = eng
    X = Y = Z = 128
    F = 16
    ctx, res = new_ctx(vx), new_ctx(vx)
    try:
        for c in (ctx, res):
            c.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, F)
        info = ctx.world_info()
        # built worlds have no spare capacity: the first creation grows the pool, by 1.5x or more
        region = (BOX, 1, (0, 96, 0), (63, 127, 63))          # 4 x 2 x 4 bricks of sky, brick aligned
        st = ctx.edit_voxels([region])
        assert st.bricks_created == 32 and st.pool_slots == info.nslots + 32
        assert st.pool_capacity >= max(int(info.nslots * 1.5), info.nslots + 32)
        # clear frees them; set again takes the same slots back: no new slots, no growth
        st_c = ctx.edit_voxels([(BOX, 0, (0, 96, 0), (63, 127, 63))])
        assert st_c.bricks_freed == 32 and st_c.bricks_created == 0 and st_c.bricks_live == info.nslots
        d_cleared = ctx.download_world()
        bw = F ** 3 // 32
        assert not d_cleared["pool"].reshape(-1, bw)[info.nslots:].any()     # freed slots are zero
        st_s = ctx.edit_voxels([region])
        assert st_s.bricks_created == 32 and (st_s.pool_slots, st_s.pool_capacity) == (st.pool_slots, st.pool_capacity)
        dense = vxo_edit.apply_edits(gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z), X, Y, Z, [region])
        w = vxo.World.from_dense(dense, X, Y, Z, F)
        assert_tables(ctx, w)
        assert_frames(vx, ctx, torch, vxo, w, cams="AB", variants=(4,))
        # after edit_reserve the same edits need no growth
        res.edit_reserve(info.nslots + 1000)
        st_r = res.edit_voxels([region])
        assert st_r.pool_capacity == info.nslots + 1000 and st_r.bricks_created == 32
        assert_tables(res, w)
        res.edit_reserve(10)                                   # never shrinks
        assert res.edit_voxels([]).pool_capacity == info.nslots + 1000
    finally:
        ctx.close()
        res.close()


def test_all_or_nothing_and_no_op_calls(eng, vxo, tmp_path):
    vx, torch = eng
    X = Y = Z = 128
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, 16)
        ctx.edit_voxels([(SPHERE, 0, (64, 40, 64), (20, 0, 0))])
        before = ctx.download_world()
        ctx.save_world(str(tmp_path / "a.vxb"))
        for bad in [(2, 1, (0, 0, 0), (5, 5, 5)), (BOX, 3, (0, 0, 0), (5, 5, 5)), (SPHERE, 1, (5, 5, 5), (-1, 0, 0)),
                    (SPHERE, 1, (5, 5, 5), (3, 0, 1))]:
            with pytest.raises(vx.VxrtError, match="error -1"):
                ctx.edit_voxels([(BOX, 1, (0, 0, 0), (127, 127, 127)), bad])
        with pytest.raises(vx.VxrtError, match="error -1"):
            ctx.edit_voxels([(BOX, 1, (0, 0, 0), (1, 1, 1))] * 1025)
        # no-ops: outside the world, empty boxes, setting solid voxels / clearing empty ones
        st = ctx.edit_voxels([(BOX, 1, (200, 0, 0), (300, 10, 10)), (BOX, 1, (9, 0, 0), (3, 10, 10)),
                              (SPHERE, 0, (-50, -50, -50), (10, 0, 0)), (BOX, 0, (0, 120, 0), (127, 127, 127)),
                              (BOX, 1, (0, 0, 0), (127, 1, 127))])
        assert st.bricks_touched > 0 and st.bricks_created == st.bricks_freed == 0
        after = ctx.download_world()
        assert all(np.array_equal(before[k], after[k]) for k in ("coarse_bits", "brick_slot", "bounds", "pool"))
        ctx.save_world(str(tmp_path / "b.vxb"))
        assert (tmp_path / "a.vxb").read_bytes() == (tmp_path / "b.vxb").read_bytes()
        # an unedited world saves exactly as before: a fresh build, saved twice, around a no-op edit
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, 16)
        ctx.save_world(str(tmp_path / "c.vxb"))
        ctx.edit_voxels([(BOX, 0, (0, 120, 0), (127, 127, 127))])
        ctx.save_world(str(tmp_path / "d.vxb"))
        assert (tmp_path / "c.vxb").read_bytes() == (tmp_path / "d.vxb").read_bytes()
    finally:
        ctx.close()


def test_refusals(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        op = (vx.EditOp * 1)(vx.EditBox((0, 0, 0), (3, 3, 3), 1))
        assert ctx._L.vxrt_edit_voxels(ctx._h, op, 1, None) == -3        # no world
        assert ctx._L.vxrt_edit_reserve(ctx._h, 100) == -3
        w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16)
        upload(ctx, w)
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert ctx._L.vxrt_edit_voxels(ctx._h, op, 1, None) == -1        # streamed world
        assert ctx._L.vxrt_edit_reserve(ctx._h, 5000) == -1
        ctx.stream_close()
    finally:
        ctx.close()


def test_compacting_save_loads_and_streams(eng, vxo, tmp_path):
    vx, torch = eng
    X = Y = Z = 256
    F = 16
    rng = np.random.default_rng(5)
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx, other = new_ctx(vx), new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, F)
        for _ in range(6):
            ops = random_ops(rng, (X, Y, Z), 30, 60)
            ctx.edit_voxels(ops)
            dense = vxo_edit.apply_edits(dense, X, Y, Z, ops)
        w = vxo.World.from_dense(dense, X, Y, Z, F)
        path = str(tmp_path / "edited.vxb")
        ctx.save_world(path)
        info = vx.world_file_info(path)
        live = int((w.brick_slot != 0xFFFFFFFF).sum())
        assert info.nslots == live
        other.load_world(path)
        d = assert_tables(other, w)
        occ = d["brick_slot"] != 0xFFFFFFFF
        assert np.array_equal(d["brick_slot"][occ], np.arange(live))     # renumbered in cell order, as the builders do
        assert np.array_equal(d["brick_slot"], w.brick_slot)
        assert_frames(vx, other, torch, vxo, w, cams="AD", variants=(4,))
        other.stream_open(path, live)
        other.stream_focus((128.0, 128.0, 128.0), 1.0e6)
        assert_tables(other, w)
        assert_frames(vx, other, torch, vxo, w, cams="A", variants=(4,))
        other.stream_close()
    finally:
        ctx.close()
        other.close()


def test_launch_before_the_edit_sees_the_old_world(eng, vxo):
    vx, torch = eng
    X = Y = Z = 128
    F = 16
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, F)
        ops = [(BOX, 0, (0, 0, 0), (127, 127, 63)), (SPHERE, 1, (64, 100, 96), (24, 0, 0))]
        old = vxo.World.from_dense(dense, X, Y, Z, F)
        new = vxo.World.from_dense(vxo_edit.apply_edits(dense, X, Y, Z, ops), X, Y, Z, F)
        side = torch.cuda.Stream()
        pos, f, u, r = helpers.camera("A", old.dims, vxo)
        opts = vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=3)
        fb0 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        fb1 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            ctx.RenderScreen(W, H, fb0, pos, f, u, r, opts)
        ctx.edit_voxels(ops)
        with torch.cuda.stream(side):
            ctx.RenderScreen(W, H, fb1, pos, f, u, r, opts)
        side.synchronize()
        want0 = oracle_frame(vxo, old, "A", old.dims, vx.MODE_SHADED)
        want1 = oracle_frame(vxo, new, "A", new.dims, vx.MODE_SHADED)
        assert not np.array_equal(want0, want1)
        assert np.array_equal(fb0.cpu().numpy(), want0) and np.array_equal(fb1.cpu().numpy(), want1)
    finally:
        ctx.close()


def test_speculative_loads_stay_in_the_slack_of_a_grown_pool(eng, vxo):
    """The slack contract (tests/test_gpu_parity.py) on this fifth world path: an edited world whose pool has grown."""
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32)
        n0 = ctx.world_info().nslots
        st = ctx.edit_voxels([(SPHERE, 1, (128, 200, 128), (40, 0, 0)), (BOX, 0, (0, 0, 0), (40, 255, 40))])
        assert st.pool_capacity > n0 and st.bricks_created > 0
        w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32)
        o, d = helpers.mixed_rays(w.dims, 200000, 3)

        def exercise():
            slack = stray = 0
            ctx.frame_stats()
            for cam in "ABCD":
                pos, f, u, r = helpers.camera(cam, w.dims, vxo)
                fb = torch.zeros((120, 200, 4), dtype=torch.uint8, device="cuda")
                ctx.RenderScreen(200, 120, fb, pos, f, u, r, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=2,
                                                                             collect_stats=True))
                s = ctx.frame_stats()
                slack, stray = slack + s.guard_slack_loads, stray + s.guard_stray_loads
            s = ctx.Raytrace(o, d, want_stats=True)["stats"]
            return slack + s.guard_slack_loads, stray + s.guard_stray_loads

        slack, stray = exercise()
        assert stray == 0 and slack > 0
        ctx.guard_pretend_no_slack(True)
        slack2, stray2 = exercise()
        ctx.guard_pretend_no_slack(False)
        assert slack2 == 0 and 0.7 * slack <= stray2 <= 1.4 * slack, (slack, stray2)
    finally:
        ctx.close()


def test_pick_and_dig(eng, vxo):
    """Raytrace hits cleared with one-voxel boxes, voxels placed at hit + normal: the next Raytrace equals the oracle."""
    vx, torch = eng
    X = Y = Z = 128
    F = 8
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(dense, X, Y, Z, F))
        rng = np.random.default_rng(3)
        o = np.tile(np.array([[64.0, 120.0, 64.0]], np.float32), (4000, 1))
        d = rng.normal(size=(4000, 3)).astype(np.float32)
        d[:, 1] = -np.abs(d[:, 1])
        for rnd in range(3):
            g = ctx.Raytrace(o, d)
            hit = g["hit"].astype(bool)
            vox = g["voxel"][hit]
            xyz = np.stack([vox % X, (vox // X) % Y, vox // (X * Y)], 1)
            nrm = g["normal"][hit].astype(np.int64)
            ops = [(BOX, 0, tuple(p), tuple(p)) for p in xyz[:400].tolist()]
            ops += [(BOX, 1, tuple(p), tuple(p)) for p in (xyz[400:800] + nrm[400:800]).tolist()]
            assert len(ops) > 100
            ctx.edit_voxels(ops)
            dense = vxo_edit.apply_edits(dense, X, Y, Z, ops)
            w = vxo.World.from_dense(dense, X, Y, Z, F)
            g2 = ctx.Raytrace(o, d)
            c = w.trace_batch(o, d, nthreads=16)
            assert np.array_equal(g2["voxel"], c["voxel"]) and np.array_equal(g2["steps"], c["steps"])
            assert np.array_equal(helpers.float_bits(g2["hitPoint"]), helpers.float_bits(c["pos"]))
        assert_tables(ctx, w)
    finally:
        ctx.close()


FACADE_EDITS = [(1, (SPHERE, 0, (150, 150, 150), (70, 0, 0))), (1, (BOX, 1, (120, 200, 120), (160, 215, 140))),
                (2, (SPHERE, 1, (110, 190, 100), (18, 0, 0))), (2, (BOX, 0, (0, 0, 0), (255, 120, 60)))]


def _facade_oracle_frames(vxo, edits, W_, H_):
    edge = 256
    dense = gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge)
    fb = np.full((H_, W_, 4), 255, np.uint8)
    frames = []
    for frame, (pos, euler) in enumerate(FACADE_POSES):
        ops = [op for fr, op in edits if fr == frame]
        if ops:
            dense = vxo_edit.apply_edits(dense, edge, edge, edge, ops)
        w = vxo.World.from_dense(dense, edge, edge, edge, 32)
        f, u, r = vxo.get_directions(euler)
        p = vxo.make_params(W_, H_, tuple(np.float32(v) for v in pos), f, u, r, frame_number=frame, mode=vxo.MODE_SHADED,
                            checkerboard=1, shadow=1, bounce_samples=1)
        fb = w.render(p, fb=fb.copy(), nthreads=16)["fb"]
        frames.append(fb)
    return frames


def test_headless_example_edit_script(vxo, tmp_path):
    """examples/voxelapp_headless with an edit script (VoxelRaytracer3D::EditVoxels before the frames it names) and a
    camera path: every dumped frame equals the oracle's frame of the world edited up to that frame."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    W_, H_ = 160, 96
    path = tmp_path / "path.txt"
    path.write_text("".join("%r %r %r %r %r %r\n" % (*p, *e) for p, e in FACADE_POSES))
    script = tmp_path / "edits.txt"
    script.write_text("# frame kind value ax ay az bx by bz\n" + "".join(
        "%d %d %d %d %d %d %d %d %d\n" % (fr, k, v, *a, *b) for fr, (k, v, a, b) in FACADE_EDITS))
    prefix = str(tmp_path / "ed")
    out = subprocess.run([exe, "256", "0", prefix, str(W_), str(H_), "1", str(path), "1", "1", "1", "0x0x0", str(script)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("edit before frame") == 2
    want = _facade_oracle_frames(vxo, FACADE_EDITS, W_, H_)
    plain = _facade_oracle_frames(vxo, [], W_, H_)
    assert not np.array_equal(want[2], plain[2])     # the edits show
    head = b"P6\n%d %d\n255\n" % (W_, H_)
    for frame in range(len(FACADE_POSES)):
        raw = open("%s_%04d.ppm" % (prefix, frame), "rb").read()
        assert raw.startswith(head)
        rgb = np.frombuffer(raw[len(head):], np.uint8).reshape(H_, W_, 3)
        assert np.array_equal(rgb, want[frame][:, :, [2, 1, 0]]), frame
