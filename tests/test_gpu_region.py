"""Region readback and voxel stamps on the device (include/vxrt.h, vxrt_read_region / vxrt_edit_stamps; extensions next to
the voxel editing).  Reads must equal the oracle's region of the world (oracle/vxo_region.c, oracle/ref_region.py); after
every stamp call the resident tables must be what the oracle's brickmap builder makes of the oracle-stamped dense grid
(slot numbers excepted), and frames and batches must equal the oracle's on that world, byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_region, vxo_edit, vxo_region
from tests import helpers
from tests.helpers import (FACADE_POSES, assert_batch, assert_frames, assert_tables, eng, gen_dense, new_ctx, oracle_frame,
                           random_ops, render_frame, upload)

pytestmark = pytest.mark.gpu
REPLACE, UNION, SUBTRACT = 0, 1, 2
BOX, SPHERE = 0, 1
W, H = 64, 48
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_box(rng, dims, maxd):
    d = [int(rng.integers(1, min(n, maxd) + 20)) for n in dims]
    if rng.random() < 0.2:
        d[0] = int(rng.choice([1, 31, 32, 33, 65]))
    o = [int(rng.integers(-30, n + 10)) for n in dims]
    return o, d


def _assert_reads(vx, ctx, vox, rng, n=40, maxd=96):
    for q in range(n):
        o, d = _random_box(rng, vox.shape, maxd)
        if q == 0:
            o, d = [-3, -4, -5], [s + 9 for s in vox.shape]   # every face
        want = ref_region.read_region(vox, o, d)
        words = ctx.read_region(o, d)
        assert words.numel() == vx.region_words(d)
        assert np.array_equal(words.cpu().numpy().view(np.uint32), vx.pack_region(want)), (o, d)  # padding bits 0
        if q % 8 == 0:
            assert np.array_equal(ctx.read_region_host(o, d), want)


WORLDS = [  # (factor, X, Y, Z, how the world is made)
    (8, 64, 64, 64, "upload"),
    (16, 128, 128, 128, "device"),
    (32, 256, 256, 256, "upload"),
    (8, 8192, 64, 64, "upload"),    # a wide grid: 1024 x 8 x 8 cells
    (16, 128, 128, 128, "file"),
    (32, 256, 256, 256, "edited"),   # freed slots, bricks out of cell order, a grown pool
]


@pytest.mark.parametrize("factor,X,Y,Z,how", WORLDS)
def test_reads_equal_the_oracle(eng, vxo, tmp_path, factor, X, Y, Z, how):
    vx, torch = eng
    rng = np.random.default_rng(factor + X + len(how))
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx = new_ctx(vx)
    try:
        if how == "upload":
            upload(ctx, vxo.World.from_dense(dense, X, Y, Z, factor))
        elif how == "device":
            ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
        elif how == "file":
            other = new_ctx(vx)
            other.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
            other.save_world(str(tmp_path / "w.vxb"))
            other.close()
            ctx.load_world(str(tmp_path / "w.vxb"))
        else:
            ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
            n0 = ctx.world_info().nslots
            for _ in range(4):
                ops = random_ops(rng, (X, Y, Z), 24, 60)
                ctx.edit_voxels(ops)
                dense = vxo_edit.apply_edits(dense, X, Y, Z, ops)
            st = ctx.edit_voxels([(SPHERE, 1, (128, 220, 128), (30, 0, 0))])
            dense = vxo_edit.apply_edits(dense, X, Y, Z, [(SPHERE, 1, (128, 220, 128), (30, 0, 0))])
            assert st.pool_capacity > n0
        vox = vxo_edit.voxels_from_dense(dense, X, Y, Z)
        _assert_reads(vx, ctx, vox, rng)
    finally:
        ctx.close()


def _bench_bricks_to_region(d, bx0, by0, bz, nbx, nby):
    """one brick layer (z = bz * 32 .. + 31) of the window, decoded from download_world's tiled tables: bool [x, y, 32]"""
    f = 32
    cx, cy, _ = d["cdims"]
    bx, by = np.meshgrid(np.arange(bx0, bx0 + nbx), np.arange(by0, by0 + nby), indexing="ij")
    t = ((bz >> 3) * (cy >> 3) + (by >> 3)) * (cx >> 3) + (bx >> 3)
    t = t * 512 + (bx & 7) + ((by & 7) << 3) + ((bz & 7) << 6)
    slot = d["brick_slot"][t.reshape(-1)]
    occ = slot != 0xFFFFFFFF
    bricks = np.zeros((slot.size, 1024), np.uint32)
    bricks[occ] = d["pool"].reshape(-1, 1024)[slot[occ]]
    bits = np.unpackbits(bricks.view(np.uint8), axis=1, bitorder="little").reshape(-1, 4, 4, 4, 8, 8, 8)  # tz ty tx z y x
    vox = bits.transpose(0, 3, 6, 2, 5, 1, 4).reshape(nbx, nby, f, f, f).astype(bool)                   # bx by x y z
    return vox.transpose(0, 2, 1, 3, 4).reshape(nbx * f, nby * f, f)


def test_reads_at_scale_on_the_bench_world(eng):
    """brick-aligned, full-height windows of at least 2^30 voxels of the device-built 8192 x 512 x 8192 world against its
    own download_world tables decoded on the host"""
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        d = ctx.download_world()
        for o, dims in [((4096, 0, 2048), (2048, 512, 1024)), ((0, 0, 7168), (8192, 512, 256))]:
            words = ctx.read_region(o, dims).cpu().numpy().view(np.uint32)
            assert words.size == dims[0] * dims[1] * dims[2] // 32 >= 1 << 25
            layer = dims[0] // 32 * dims[1] * 32        # words of one brick layer (32 z)
            solid = 0
            for k in range(dims[2] // 32):
                want = _bench_bricks_to_region(d, o[0] // 32, 0, o[2] // 32 + k, dims[0] // 32, 16)
                assert np.array_equal(words[k * layer:(k + 1) * layer], vx.pack_region(want)), k
                solid += int(want.sum())
            assert solid > 0
    finally:
        ctx.close()


def _random_stamp(rng, dims, maxd, ctx, src_vox):
    """(origin, bool mask, mode, device words or None): a random mask, or a copy of a region of the world as it is"""
    o, d = _random_box(rng, dims, maxd)
    mode = int(rng.integers(0, 3))
    if rng.random() < 0.3:
        so = [int(rng.integers(-10, n)) for n in dims]
        words = ctx.read_region(so, d)
        return o, ref_region.read_region(src_vox, so, d), mode, words
    kind = rng.random()
    if kind < 0.4:
        m = rng.random(d) < rng.random()
    elif kind < 0.7:                                      # a ball
        g = np.indices(d).astype(np.float64)
        c = [s / 2 for s in d]
        m = ((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) <= (min(d) / 2) ** 2
    else:
        m = np.full(d, rng.random() < 0.5)
    return o, m, mode, None


@pytest.mark.parametrize("factor,X,Y,Z,how", WORLDS[:4])
def test_random_stamp_sequences_equal_the_oracle(eng, vxo, factor, X, Y, Z, how):
    vx, torch = eng
    rng = np.random.default_rng(factor * 3 + X)
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx, twin = new_ctx(vx), new_ctx(vx)
    try:
        for c in (ctx, twin):
            if how == "device":
                c.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, factor)
            else:
                upload(c, vxo.World.from_dense(dense, X, Y, Z, factor))
        created = freed = 0
        modes = set()
        for call in range(12):
            vox = vxo_edit.voxels_from_dense(dense, X, Y, Z)
            stamps = [_random_stamp(rng, (X, Y, Z), max(min(X, Y, Z), 32), ctx, vox) for _ in range(int(rng.integers(1, 7)))]
            modes |= {s[2] for s in stamps}
            st = ctx.edit_stamps([vx.Stamp(o, w if w is not None else m, mode, m.shape) for o, m, mode, w in stamps])
            st2 = twin.edit_stamps([vx.Stamp(o, m, mode) for o, m, mode, _ in stamps])
            dense = vxo_region.apply_stamps(dense, X, Y, Z, [(o, vx.pack_region(m), m.shape, mode) for o, m, mode, _ in stamps])
            assert np.array_equal(vxo_edit.voxels_from_dense(dense, X, Y, Z), ref_region.apply_stamps(vox, [s[:3] for s in stamps]))
            w = vxo.World.from_dense(dense, X, Y, Z, factor)
            d = assert_tables(ctx, w)
            assert st.bricks_live == int((w.brick_slot != 0xFFFFFFFF).sum())
            created, freed = created + st.bricks_created, freed + st.bricks_freed
            d2 = twin.download_world()      # determinism: the same calls give byte-identical downloads, pool included
            assert all(np.array_equal(d[k], d2[k]) for k in ("coarse_bits", "brick_slot", "bounds", "pool"))
            assert (st.bricks_created, st.bricks_freed, st.pool_slots) == (st2.bricks_created, st2.bricks_freed, st2.pool_slots)
            full = call % 4 == 3
            assert_frames(vx, ctx, torch, vxo, w, cams="ABCD" if full else "A", variants=(4, 1) if full else (4,))
            if full:
                assert_batch(ctx, w, seed=call)
        assert created > 0 and freed > 0 and modes == {0, 1, 2}
    finally:
        ctx.close()
        twin.close()


@pytest.mark.parametrize("side_stream", [False, True])
def test_undo_restores_tables_and_frames(eng, vxo, side_stream):
    """read a box, edit inside it, stamp the read back with replace: the original world (tables, slot numbers excepted)
    and byte-identical frames; with side_stream the read runs on another stream and nothing synchronises explicitly"""
    vx, torch = eng
    X = Y = Z = 256
    F = 32
    rng = np.random.default_rng(9 + side_stream)
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    w0 = vxo.World.from_dense(dense, X, Y, Z, F)
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, F)
        frames0 = {(cam, m): oracle_frame(vxo, w0, cam, w0.dims, m) for cam in "ABCD" for m in (vx.MODE_SHADED, vx.MODE_DEBUG)}
        changed = 0
        for rnd in range(3):
            lo = [int(rng.integers(0, 128)) for _ in range(3)]
            dims = [int(rng.integers(40, 128)) for _ in range(3)]
            if side_stream:
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):
                    saved = ctx.read_region(lo, dims)
            else:
                saved = ctx.read_region(lo, dims)
            ops = []
            for _ in range(int(rng.integers(5, 30))):
                a = [l + int(rng.integers(0, d)) for l, d in zip(lo, dims)]
                if rng.random() < 0.5:
                    b = [min(v + int(rng.integers(0, 20)), l + d - 1) for v, l, d in zip(a, lo, dims)]
                    ops.append((BOX, int(rng.integers(0, 2)), a, b))
                else:
                    r = min(int(rng.integers(0, 16)), *[min(v - l, l + d - 1 - v) for v, l, d in zip(a, lo, dims)])
                    ops.append((SPHERE, int(rng.integers(0, 2)), a, (r, 0, 0)))
            ctx.edit_voxels(ops)
            edited = vxo_edit.voxels_from_dense(vxo_edit.apply_edits(dense, X, Y, Z, ops), X, Y, Z)
            assert np.array_equal(ctx.read_region_host(lo, dims), ref_region.read_region(edited, lo, dims))
            changed += int(not np.array_equal(edited, vxo_edit.voxels_from_dense(dense, X, Y, Z)))
            ctx.edit_stamps([vx.Stamp(lo, saved, REPLACE, dims)])
            assert_tables(ctx, w0)
            for cam in "ABCD":
                for m in (vx.MODE_SHADED, vx.MODE_DEBUG):
                    assert np.array_equal(render_frame(vx, ctx, torch, cam, w0.dims, vxo, m), frames0[(cam, m)]), (rnd, cam, m)
        assert changed > 0
    finally:
        ctx.close()


def test_copy_paste_apart_and_overlapping(eng, vxo):
    vx, torch = eng
    X = Y = Z = 128
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    vox = vxo_edit.voxels_from_dense(dense, X, Y, Z)
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, 16)
        src, dims = (10, 20, 30), (40, 50, 35)
        clip = ctx.read_region(src, dims)
        ctx.edit_stamps([vx.Stamp((70, 60, 5), clip, REPLACE, dims)])                      # apart
        want = vox.copy()
        want[70:110, 60:110, 5:40] = vox[10:50, 20:70, 30:65]
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (X, Y, Z)), want)
        clip2 = ctx.read_region(src, dims)
        ctx.edit_stamps([vx.Stamp((25, 30, 40), clip2, REPLACE, dims)])                    # overlapping its source
        want2 = want.copy()
        want2[25:65, 30:80, 40:75] = want[10:50, 20:70, 30:65]
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (X, Y, Z)), want2)
        ctx.edit_stamps([vx.Stamp((100, 100, 100), clip2, UNION, dims)])                   # clipped at the far faces
        want3 = want2.copy()
        want3[100:, 100:, 100:] |= want[10:38, 20:48, 30:58]
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (X, Y, Z)), want3)
        assert_tables(ctx, vxo.World.from_dense(vxo.dense_from_voxels(want3), X, Y, Z, 16))
    finally:
        ctx.close()


def _descs(vx, stamps):
    arr = (vx.StampDesc * max(len(stamps), 1))()
    for i, (ptr, o, d, mode, res) in enumerate(stamps):
        arr[i].d_bits = ptr
        arr[i].origin = (C.c_int32 * 3)(*o)
        arr[i].dims = (C.c_int32 * 3)(*d)
        arr[i].mode, arr[i].reserved = mode, res
    return arr


def test_all_or_nothing_and_zero_union(eng, vxo, tmp_path):
    vx, torch = eng
    X = Y = Z = 128
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, 16)
        ctx.edit_voxels([(SPHERE, 0, (64, 40, 64), (20, 0, 0))])          # freed slots: the world was edited
        before = ctx.download_world()
        ones = torch.full((4 * 64 * 64,), -1, dtype=torch.int32, device="cuda")
        good = (ones.data_ptr(), (0, 0, 0), (128, 64, 64), REPLACE, 0)
        for k, bad in enumerate([(ones.data_ptr(), (0, 0, 0), (128, 64, 64), 3, 0),
                                 (ones.data_ptr(), (0, 0, 0), (128, 64, 64), UNION, 1),
                                 (ones.data_ptr(), (0, 0, 0), (0, 64, 64), UNION, 0),
                                 (ones.data_ptr(), (0, 0, 0), (4096, 4096, 4097), UNION, 0),
                                 (None, (0, 0, 0), (128, 64, 64), UNION, 0)]):
            stamps = [good] * (k + 1) + [bad]
            assert ctx._L.vxrt_edit_stamps(ctx._h, _descs(vx, stamps), len(stamps), None) == -1, k
        assert ctx._L.vxrt_edit_stamps(ctx._h, _descs(vx, [good] * 1025), 1025, None) == -1
        after = ctx.download_world()
        assert all(np.array_equal(before[k], after[k]) for k in ("coarse_bits", "brick_slot", "bounds", "pool"))
        # a union (or subtract) of an all-zero mask touches bricks and changes nothing: nothing written
        zero = torch.zeros(4 * 128 * 128, dtype=torch.int32, device="cuda")
        for mode in (UNION, SUBTRACT):
            st = ctx.edit_stamps([vx.Stamp((0, 0, 0), zero, mode, (128, 128, 128))])
            assert st.bricks_touched == 512 and st.bricks_created == st.bricks_freed == 0
            assert st.pool_slots == before["pool"].size // (16 ** 3 // 32)
        after = ctx.download_world()
        assert all(np.array_equal(before[k], after[k]) for k in ("coarse_bits", "brick_slot", "bounds", "pool"))
        # a replace with the world's own voxels changes nothing either
        st = ctx.edit_stamps([vx.Stamp((0, 0, 0), ctx.read_region((0, 0, 0), (X, Y, Z)), REPLACE, (X, Y, Z))])
        assert st.bricks_created == st.bricks_freed == 0
        assert all(np.array_equal(before[k], ctx.download_world()[k]) for k in ("coarse_bits", "brick_slot", "bounds", "pool"))
    finally:
        ctx.close()


def test_refusals(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
        o3, d3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
        host = np.zeros(64, np.uint32)
        st = _descs(vx, [(buf.data_ptr(), (0, 0, 0), (8, 8, 8), REPLACE, 0)])
        assert ctx._L.vxrt_read_region(ctx._h, o3, d3, buf.data_ptr(), None) == -3         # no world
        assert ctx._L.vxrt_read_region_host(ctx._h, o3, d3, host.ctypes.data) == -3
        assert ctx._L.vxrt_edit_stamps(ctx._h, st, 1, None) == -3
        w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16)
        upload(ctx, w)
        for bad in [(0, 8, 8), (8, -1, 8), (4096, 4096, 4097)]:                                  # bad dims
            assert ctx._L.vxrt_read_region(ctx._h, o3, (C.c_int32 * 3)(*bad), buf.data_ptr(), None) == -1
            assert ctx._L.vxrt_read_region_host(ctx._h, o3, (C.c_int32 * 3)(*bad), host.ctypes.data) == -1
        assert ctx._L.vxrt_read_region(ctx._h, o3, d3, None, None) == -1                          # NULL pointers
        assert ctx._L.vxrt_read_region(ctx._h, None, d3, buf.data_ptr(), None) == -1
        assert ctx._L.vxrt_read_region(ctx._h, o3, None, buf.data_ptr(), None) == -1
        assert ctx._L.vxrt_read_region_host(ctx._h, o3, d3, None) == -1
        assert ctx._L.vxrt_edit_stamps(ctx._h, None, 1, None) == -1
        assert ctx._L.vxrt_edit_stamps(ctx._h, None, 0, None) == 0                                # an empty list is a no-op
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert ctx._L.vxrt_read_region(ctx._h, o3, d3, buf.data_ptr(), None) == -1               # streamed world
        assert ctx._L.vxrt_read_region_host(ctx._h, o3, d3, host.ctypes.data) == -1
        assert ctx._L.vxrt_edit_stamps(ctx._h, st, 1, None) == -1
        ctx.stream_close()
    finally:
        ctx.close()


def test_a_strided_out_is_refused_and_left_unchanged(eng, vxo):
    """read_region writes dense words through ``out``'s address: an ``out`` with a stride is refused before the library is
    called, and its dense half is accepted (64^3 is the smallest world of factor 8: 8 coarse cells per axis)"""
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        vox = np.random.default_rng(21).random((64, 64, 64)) < 0.4
        upload(ctx, vxo.World.from_voxels(vox, 8))
        o, d = (28, 27, 26), (8, 8, 8)
        n = vx.region_words(d)
        buf = torch.full((2 * n,), 0x1234, dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError):
            ctx.read_region(o, d, out=buf[::2])
        torch.cuda.synchronize()
        assert bool((buf == 0x1234).all())
        got = ctx.read_region(o, d, out=buf[:n])
        assert np.array_equal(vx.unpack_region(got, d), vox[28:36, 27:35, 26:34]) and bool((buf[n:] == 0x1234).all())
    finally:
        ctx.close()


def test_read_after_render_on_a_stream_sees_the_renders_world(eng, vxo):
    vx, torch = eng
    X = Y = Z = 128
    F = 16
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, X, Y, Z)
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, X, Y, Z, F)
        ops = [(BOX, 0, (0, 0, 0), (127, 127, 63)), (SPHERE, 1, (64, 100, 96), (24, 0, 0))]
        new_dense = vxo_edit.apply_edits(dense, X, Y, Z, ops)
        old, new = vxo.World.from_dense(dense, X, Y, Z, F), vxo.World.from_dense(new_dense, X, Y, Z, F)
        side = torch.cuda.Stream()
        pos, f, u, r = helpers.camera("A", old.dims, vxo)
        opts = vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=3)
        fb0 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        fb1 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            ctx.RenderScreen(W, H, fb0, pos, f, u, r, opts)
            r0 = ctx.read_region((0, 0, 0), (X, Y, Z))
        ctx.edit_voxels(ops)
        with torch.cuda.stream(side):
            ctx.RenderScreen(W, H, fb1, pos, f, u, r, opts)
            r1 = ctx.read_region((0, 0, 0), (X, Y, Z))
        side.synchronize()
        assert np.array_equal(fb0.cpu().numpy(), oracle_frame(vxo, old, "A", old.dims, vx.MODE_SHADED))
        assert np.array_equal(fb1.cpu().numpy(), oracle_frame(vxo, new, "A", new.dims, vx.MODE_SHADED))
        assert np.array_equal(vx.unpack_region(r0, (X, Y, Z)), vxo_edit.voxels_from_dense(dense, X, Y, Z))
        assert np.array_equal(vx.unpack_region(r1, (X, Y, Z)), vxo_edit.voxels_from_dense(new_dense, X, Y, Z))
    finally:
        ctx.close()


def test_speculative_loads_stay_in_the_slack_of_a_pool_grown_by_stamps(eng, vxo):
    """The slack contract (tests/test_gpu_parity.py) on a world whose pool grew through vxrt_edit_stamps."""
    vx, torch = eng
    ctx = new_ctx(vx)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32)
        n0 = ctx.world_info().nslots
        rng = np.random.default_rng(1)
        st = ctx.edit_stamps([vx.Stamp((20, 150, 30), rng.random((200, 90, 180)) < 0.02, UNION),
                              vx.Stamp((0, 0, 0), np.zeros((40, 256, 40), bool), REPLACE)])
        assert st.pool_capacity > n0 and st.bricks_created > 0 and st.bricks_freed > 0
        w = vxo.World.generate(vxo.GEN_INT_TERRAIN, 256, 256, 256, 32)
        o, d = helpers.mixed_rays(w.dims, 200000, 3)
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
        slack, stray = slack + s.guard_slack_loads, stray + s.guard_stray_loads
        assert stray == 0 and slack > 0
    finally:
        ctx.close()


# frame, kind, value, a, b: kind 2 = copy box (a, dims b) into slot value, kind 3 = paste slot value at a in mode b[0]
FACADE_SCRIPT = [(1, 2, 0, (100, 100, 100), (60, 90, 50)), (1, 0, 0, (90, 150, 90), (200, 255, 200)),
                 (1, 3, 0, (150, 165, 120), (0, 0, 0)), (2, 3, 0, (40, 170, 30), (1, 0, 0)),
                 (2, 2, 1, (0, 0, 0), (256, 256, 256)), (2, 1, 0, (128, 128, 128), (60, 0, 0)),
                 (2, 3, 1, (10, 5, -3), (2, 0, 0))]


def _script_oracle_frames(vxo, W_, H_):
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    clips = {}
    fb = np.full((H_, W_, 4), 255, np.uint8)
    frames = []
    from oracle import ref_edit
    for frame, (pos, euler) in enumerate(FACADE_POSES):
        for fr, kind, value, a, b in FACADE_SCRIPT:
            if fr != frame:
                continue
            if kind == 2:
                clips[value] = ref_region.read_region(vox, a, b)
            elif kind == 3:
                vox = ref_region.apply_stamps(vox, [(a, clips[value], b[0])])
            else:
                vox = ref_edit.apply_edits(vox, [(kind, value, a, b)])
        w = vxo.World.from_dense(vxo.dense_from_voxels(vox), edge, edge, edge, 32)
        f, u, r = vxo.get_directions(euler)
        p = vxo.make_params(W_, H_, tuple(np.float32(v) for v in pos), f, u, r, frame_number=frame, mode=vxo.MODE_SHADED,
                            checkerboard=1, shadow=1, bounce_samples=1)
        fb = w.render(p, fb=fb.copy(), nthreads=16)["fb"]
        frames.append(fb)
    return frames


def test_headless_example_copy_paste_script(vxo, tmp_path):
    """examples/voxelapp_headless with an edit script of copy (kind 2) and paste (kind 3) lines mixed with shape ops:
    every dumped frame equals the oracle's frame of the world edited up to that frame"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    W_, H_ = 160, 96
    path = tmp_path / "path.txt"
    path.write_text("".join("%r %r %r %r %r %r\n" % (*p, *e) for p, e in FACADE_POSES))
    script = tmp_path / "edits.txt"
    script.write_text("# frame kind value ax ay az bx by bz\n" + "".join(
        "%d %d %d %d %d %d %d %d %d\n" % (fr, k, v, *a, *b) for fr, k, v, a, b in FACADE_SCRIPT))
    prefix = str(tmp_path / "cp")
    out = subprocess.run([exe, "256", "0", prefix, str(W_), str(H_), "1", str(path), "1", "1", "1", "0x0x0", str(script)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("copy before frame") == 2 and out.stdout.count("paste before frame") == 3
    want = _script_oracle_frames(vxo, W_, H_)
    head = b"P6\n%d %d\n255\n" % (W_, H_)
    for frame in range(len(FACADE_POSES)):
        raw = open("%s_%04d.ppm" % (prefix, frame), "rb").read()
        assert raw.startswith(head)
        rgb = np.frombuffer(raw[len(head):], np.uint8).reshape(H_, W_, 3)
        assert np.array_equal(rgb, want[frame][:, :, [2, 1, 0]]), frame
    assert not np.array_equal(want[2], want[0])
