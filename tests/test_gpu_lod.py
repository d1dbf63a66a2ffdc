"""The occupancy LOD on the device (include/vxrt.h, vxrt_downsample_region): bits, counts and summary equal to
tests/ref_lod.py bit for bit -- at every shift with output widths around a word and a wave and source rows around a wave of
words, on unaligned, negative and past-the-far-face origins, at densities that carry between the SWAR stages and that fill
every count, with counts given and NULL, device and host forms, two calls bit-identical, guard words behind both outputs, on
every world path the region tests use, after edits, stamps and pool growth, on a bench-world window, at the source limit of
2^32 voxels; the LOD world (Context.lod_world) built, refreshed after an edit and downsampled again; refusals in the order
of the call rules; and the headless example's lod lines (the C++ facade)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region, vxo_edit
from tests import ref_lod as R
from tests.helpers import eng, gen_dense, new_ctx, random_ops, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = (1, 2, 3, 4, 5)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
GUARD = 0x5A5A5A5A
BOX, SPHERE = 0, 1


def _summary(words):
    w = [int(x) for x in words]
    return (w[0] | w[1] << 32, w[2], w[3], w[4], w[5], w[6])


def _u32(t):
    return t.cpu().numpy().view(np.uint32) if hasattr(t, "cpu") else np.asarray(t).view(np.uint32)


def _want(world, origin, dims, shift, threshold, at=(0, 0, 0)):
    """the reference on `world`, whose voxel (0, 0, 0) is world voxel `at`: the reshape restatement, which touches the source
    box only, or the prefix sums where the source box is far larger than the world"""
    o = tuple(int(a) - int(b) for a, b in zip(origin, at))
    small = (dims[0] * dims[1] * dims[2]) << (3 * shift) <= 1 << 26
    return R.downsample(world, o, dims, shift, threshold, (R.counts_reshape if small else R.counts_prefix)(world, o, dims, shift))


def _assert_device(got, want, what, counts=True):
    print("lod", what, tuple(got.summary), _summary(want.summary))
    assert tuple(got.summary) == _summary(want.summary), what
    assert np.array_equal(_u32(got.bits), want.words), what
    if counts:
        assert np.array_equal(got.counts.cpu().numpy().view(np.uint16), want.flat), what
    else:
        assert got.counts is None


def _assert_host(got, want, what):
    assert tuple(got.summary) == _summary(want.summary), what
    assert got.bits.dtype == bool and np.array_equal(got.bits, want.bits), what
    assert got.counts.dtype == np.uint16 and np.array_equal(got.counts, want.counts), what


def _assert_lod(ctx, world, origin, dims, shift, threshold, at=(0, 0, 0), host=False, counts=True):
    want = _want(world, origin, dims, shift, threshold, at)
    got = ctx.downsample(origin, dims, shift, threshold, counts=counts)
    _assert_device(got, want, (origin, dims, shift, threshold), counts)
    if host:
        _assert_host(ctx.downsample_host(origin, dims, shift, threshold), want, ("host", origin, dims, shift, threshold))
    return got, want


def _thresholds(shift):
    full = 1 << (3 * shift)
    return [1, full // 2, full, 2, full - 1]


@pytest.fixture(scope="module")
def long_world(vxo):
    """2112 x 64 x 64 voxels (33 tiles of 64), density 0.85: the fields carry between the SWAR stages"""
    vox = np.random.default_rng(31).random((2112, 64, 64)) < 0.85
    return vxo.World.from_voxels(vox, 8), vox


@pytest.mark.parametrize("shift", SHIFTS)
def test_output_widths_around_a_word_and_a_wave(eng, long_world, shift):
    """dims[0] of 1, 31, 32, 33, 64 and 65 at origins that are unaligned, negative and past the world's far faces; device and
    host forms; counts given and NULL; two calls bit-identical"""
    vx, torch = eng
    w, vox = long_world
    f = 1 << shift
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        ts = _thresholds(shift)
        for i, nx in enumerate((1, 31, 32, 33, 64, 65)):
            origins = [(0, 0, 0), (-1, -2, -3), (2112 - f * nx // 2 - 1, 64 - f - 1, 64 - f - 3), (29, 3, 5)]
            for k, o in enumerate(origins):
                d = (nx, 3, 2)
                got, want = _assert_lod(ctx, vox, o, d, shift, ts[(i + k) % len(ts)], host=k == 1, counts=k != 2)
                again = ctx.downsample(o, d, shift, ts[(i + k) % len(ts)], counts=k != 2)
                assert again.summary == got.summary and torch.equal(again.bits, got.bits)
                assert k == 2 or torch.equal(again.counts, got.counts)
            assert want.summary[6] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("shift", SHIFTS)
def test_source_rows_around_a_wave_of_words(eng, long_world, shift):
    """source rows of 63, 64 and 65 words (f * dims[0] of 2016, 2048 and 2080), two cells along y and z"""
    vx, torch = eng
    w, vox = long_world
    f = 1 << shift
    ctx = vx.Context(0)
    try:
        upload(ctx, w)
        for sx in (2016, 2048, 2080):
            _assert_lod(ctx, vox, (17, 64 - 2 * f - 1 if f < 32 else 3, 0), (sx // f, 2, 2), shift, 1 << (3 * shift - 1))
    finally:
        ctx.close()


@pytest.mark.parametrize("shift", SHIFTS)
def test_a_solid_world_fills_every_count(eng, vxo, shift):
    """density 1.0: every cell inside the world counts f^3, the accumulators' slots at their maximum; ALL and ANY differ only
    in the cells that straddle a face"""
    vx, torch = eng
    f, full = 1 << shift, 1 << (3 * shift)
    vox = np.ones((256, 64, 64), bool)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        d = (256 // f + 2, 64 // f + 1, 64 // f + 1)
        got, want = _assert_lod(ctx, vox, (0, 0, 0), d, shift, full, host=True)
        assert got.summary.full == (256 // f) * (64 // f) ** 2 == got.summary.set and got.summary.max_count == full and got.summary.mixed == 0
        got, want = _assert_lod(ctx, vox, (-1, -1, -1), d, shift, full)
        assert got.summary.mixed > 0 and got.summary.solid == 256 * 64 * 64
        any_, _ = _assert_lod(ctx, vox, (-1, -1, -1), d, shift, 1)
        assert any_.summary.set == got.summary.set + got.summary.mixed
    finally:
        ctx.close()


def test_guard_words_behind_both_outputs(eng, vxo):
    """odd dims[0]: the uint16 tail of the counts is odd; nothing is written behind region_words(dims) words and
    dims[0] * dims[1] * dims[2] counts, and nothing at all to the counts of a call that gives none"""
    vx, torch = eng
    rng = np.random.default_rng(5)
    vox = rng.random((128, 64, 64)) < 0.5
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        L, h = ctx._L, ctx._h
        for shift in SHIFTS:
            for d in [(3, 3, 3), (33, 1, 1), (1, 1, 1), (35, 3, 1)]:
                o = (-3, 1, 2)
                nw, nc = -(-d[0] // 32) * d[1] * d[2], d[0] * d[1] * d[2]
                for counts in (True, False):
                    work = torch.zeros(ctx.lod_workspace_bytes(d, shift), dtype=torch.uint8, device="cuda")
                    bits = torch.full((nw + 8,), GUARD, dtype=torch.int32, device="cuda")
                    cnt = torch.full((nc + 9,), 0x5A5A, dtype=torch.int16, device="cuda")
                    summ = torch.zeros(8, dtype=torch.int32, device="cuda")
                    rc = L.vxrt_downsample_region(h, (C.c_int32 * 3)(*o), (C.c_int32 * 3)(*d), shift, 2, work.data_ptr(), bits.data_ptr(),
                                                  cnt.data_ptr() if counts else None, summ.data_ptr(), None)
                    assert rc == 0
                    torch.cuda.synchronize()
                    want = _want(vox, o, d, shift, 2)
                    b, c = _u32(bits), cnt.cpu().numpy().view(np.uint16)
                    assert np.array_equal(b[:nw], want.words) and (b[nw:] == GUARD).all(), (shift, d)
                    assert _summary(_u32(summ)) == _summary(want.summary)
                    if counts:
                        assert np.array_equal(c[:nc], want.flat) and (c[nc:] == 0x5A5A).all(), (shift, d)
                    else:
                        assert (c == 0x5A5A).all()
    finally:
        ctx.close()


WORLDS = [  # (factor, X, Y, Z, how the world is made): the world paths of tests/test_gpu_region.py
    (8, 64, 64, 64, "upload"),
    (16, 128, 128, 128, "device"),
    (32, 256, 256, 256, "upload"),
    (8, 8192, 64, 64, "upload"),    # a wide grid: 1024 x 8 x 8 cells
    (16, 128, 128, 128, "file"),
    (32, 256, 256, 256, "edited"),   # freed slots, bricks out of cell order, a grown pool
]


@pytest.mark.parametrize("factor,X,Y,Z,how", WORLDS)
def test_lod_on_every_world_path(eng, vxo, tmp_path, factor, X, Y, Z, how):
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
        for shift in SHIFTS:
            f = 1 << shift
            whole = tuple(-(-n // f) + 1 for n in (min(X, 512), Y, Z))  # the world (512 voxels of a wide one) and beyond it
            got, want = _assert_lod(ctx, vox, (-3, -1, -2), whole, shift, _thresholds(shift)[shift % 3])
            assert got.summary.solid > 1000
            if X > 512:
                _assert_lod(ctx, vox, (X - 200, -1, 3), (-(-230 // f), 64 // f, 64 // f), shift, 1)
    finally:
        ctx.close()


def test_lod_follows_edits_and_stamps(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(7)
    vox = rng.random((128, 128, 128)) < 0.02
    vox[:, 0, :] = True
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (-4, 0, 3), (31, 15, 28)
        before = ctx.downsample(o, d, 2).summary
        ops = [(0, 0, (0, 1, 0), (127, 40, 127)), (0, 1, (30, 1, 0), (31, 6, 100)), (1, 1, (90, 10, 90), (8, 0, 0))]
        # no synchronisation between the edits and the call: it orders after the work queued on the stream
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == 0 else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        stamps = [((10, 1, 10), rng.random((50, 3, 70)) < 0.2, vx.STAMP_UNION), ((40, 0, 40), np.zeros((20, 1, 20), bool), vx.STAMP_REPLACE)]
        ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        vox = ref_region.apply_stamps(ref_edit.apply_edits(vox, ops), stamps)
        for t in (1, 8, 64):
            got, want = _assert_lod(ctx, vox, o, d, 2, t)
        assert got.summary != before and got.summary.solid > 1000
    finally:
        ctx.close()


def _surface_y(ctx, ox, oz, below):
    """as tests/test_gpu_dist.py finds its window: the median height of a 256 x 256 patch of columns, less `below`"""
    col = ctx.read_region_host((ox, 0, oz), (256, 512, 256))
    heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
    return max(int(np.median(heights)) - below, 0)


def test_bench_world_window(eng):
    """a 256 x 128 x 256 window of the bench world at its surface, unaligned, at every shift, against the reference on
    read_region_host of the window"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz = 4001, 3003
        at = (ox, _surface_y(ctx, ox, oz, 64) + 1, oz)
        world = ctx.read_region_host(at, (256, 128, 256))
        for shift in SHIFTS:
            f = 1 << shift
            got, want = _assert_lod(ctx, world, at, (256 // f, 128 // f, 256 // f), shift, _thresholds(shift)[shift % 2], at=at)
            assert got.summary.solid == int(world.sum())
        assert want.summary[0] > 100000
    finally:
        ctx.close()


# ---- the LOD world --------------------------------------------------------------------------------------------------------
def _padded(grid, shape):
    out = np.zeros(shape, bool)
    out[:grid.shape[0], :grid.shape[1], :grid.shape[2]] = grid
    return out


def test_lod_world_built_refreshed_and_downsampled_again(eng, vxo):
    """lod_world(shift, ANY) equals the reference, cell for cell, and is empty beyond the cells that meet the world; after an
    edit lod_world(into=, box=) makes it equal again and leaves the cells outside the grown box alone (a sentinel voxel
    stamped into the LOD world stays); downsampling the LOD world by b equals the direct a + b downsample"""
    vx, torch = eng
    rng = np.random.default_rng(12)
    vox = rng.random((256, 128, 192)) < 0.003
    vox[:, :3, :] = True
    ctx = vx.Context(0)
    lod = None
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        a, f = 2, 4
        cells = (64, 32, 48)
        lod = ctx.lod_world(a, slab_cells=7)  # 48 cells along z in slabs of 7: the last one cut short
        info = lod.world_info()
        assert info.factor == 8 and tuple(info.cdims) == (8, 8, 8)
        want = _want(vox, (0, 0, 0), cells, a, 1)
        assert np.array_equal(lod.read_region_host((0, 0, 0), (64, 64, 64)), _padded(want.bits, (64, 64, 64)))
        assert 0 < want.summary[2] < want.bits.size
        # an edit, its box unaligned to f; the sentinel sits in an empty cell next to the grown box
        lo, hi = (41, 50, 61), (78, 70, 99)
        ctx.edit_voxels([vx.EditBox(lo, hi, 1), vx.EditSphere((60, 60, 80), 9, 0)])
        vox = ref_edit.apply_edits(vox, [(BOX, 1, lo, hi), (SPHERE, 0, (60, 60, 80), (9, 0, 0))])
        want = _want(vox, (0, 0, 0), cells, a, 1)
        x = hi[0] // f + 1  # the first column of cells beyond the grown box
        sentinel = next((x, y, z) for y in range(12, 18) for z in range(15, 25) if not want.bits[x, y, z])
        lod.edit_stamps([vx.Stamp(sentinel, np.ones((1, 1, 1), bool), vx.STAMP_UNION)])
        assert ctx.lod_world(a, into=lod, box=(lo, hi)) is lod
        expect = _padded(want.bits, (64, 64, 64))
        expect[sentinel] = True
        assert np.array_equal(lod.read_region_host((0, 0, 0), (64, 64, 64)), expect)
        assert ctx.lod_world(a, into=lod) is lod  # the whole world again: the sentinel goes
        assert np.array_equal(lod.read_region_host((0, 0, 0), (64, 64, 64)), _padded(want.bits, (64, 64, 64)))
        for b in (1, 2, 3):
            d = tuple(-(-n >> b) for n in cells)
            again = lod.downsample((0, 0, 0), d, b, 1)
            direct = ctx.downsample((0, 0, 0), d, a + b, 1)
            assert torch.equal(again.bits, direct.bits) and again.summary.set == direct.summary.set > 0
            _assert_device(direct, _want(vox, (0, 0, 0), d, a + b, 1), ("direct", a + b), counts=False)
        with pytest.raises(ValueError):
            ctx.lod_world(a, box=(lo, hi))
        with pytest.raises(ValueError):
            ctx.lod_world(0)
        with pytest.raises(ValueError):
            ctx.lod_world(a + 1, into=lod)  # the same size after rounding to 8 bricks, but made at shift a
        with pytest.raises(ValueError):
            ctx.lod_world(a, into=ctx)  # not an LOD world of this one: the size differs
        with pytest.raises(ValueError):
            ctx.lod_world(a, slab_cells=0)  # the context opened for it is closed again
    finally:
        if lod is not None:
            lod.close()
        ctx.close()


def _reduce_waves(dims, shift):
    """the waves of the plain reduce kernel (vxrt_lod.hpp, lod_layout): a cell row takes L lanes, the source row's words
    rounded up to a power of two up to 64; a wave task is 64 lanes; a wave takes 16, 4 or 1 tasks in turn by shift"""
    wps = -(-(dims[0] << shift) // 32)
    L = 1
    while L < wps and L < 64:
        L *= 2
    tasks = -(-wps // 64) * -(-dims[1] * dims[2] // (64 // L))
    return -(-tasks // {1: 16, 2: 4}.get(shift, 1))


def _assert_lod_of_the_part_inside(torch, ctx, vox, o, dims, shift, threshold, inside):
    """_assert_lod with counts NULL for a box of 2^26 cells and more, which the reference cannot hold: the reference over the
    cells `inside` that meet the world, the bits compared on the device with every word beyond them 0, and the summary the
    reference's with the cells beyond the world counted empty"""
    want = _want(vox, o, inside, shift, threshold)
    got = ctx.downsample(o, dims, shift, threshold, counts=False)
    s = list(_summary(want.summary))
    s[2] += dims[0] * dims[1] * dims[2] - inside[0] * inside[1] * inside[2]
    print("lod", (o, dims, shift, threshold), tuple(got.summary), tuple(s))
    assert tuple(got.summary) == tuple(s) and got.counts is None
    wpo, wpi = -(-dims[0] // 32), -(-inside[0] // 32)
    expect = torch.zeros((dims[2], dims[1], wpo), dtype=torch.int32, device="cuda")
    expect[:inside[2], :inside[1], :wpi] = torch.from_numpy(want.words.view(np.int32).reshape(inside[2], inside[1], wpi)).cuda()
    assert torch.equal(got.bits.view(dims[2], dims[1], wpo), expect)
    return got, want


SOURCE_LIMIT = [(5, (64, 64, 32)), (4, (128, 64, 128)), (3, (256, 128, 256)), (2, (256, 256, 1024)), (1, (512, 1024, 1024))]
# beside the limit: S = 2^32 makes every side a power of two and the waves a multiple of four
IDLE_WAVES = [(2, (256, 255, 1023)), (1, (512, 1023, 1023))]


@pytest.mark.parametrize("shift,dims", SOURCE_LIMIT + IDLE_WAVES)
def test_one_call_at_the_source_limit(eng, vxo, shift, dims):
    """S = 2^32 voxels (a 512 MiB workspace), mostly outside the world, counts NULL: the summary equals the reference's over
    the part inside the world and the bits beyond the world are 0.  With 2048 wave tasks and more, these are also the calls
    that take the plain kernel at shifts 4 and 5, where every smaller box of this file takes the one that splits a cell
    over a workgroup's waves.  At shifts 1 and 2 a wave takes 16 and 4 tasks in turn; the boxes of IDLE_WAVES, a cell row
    and a slice short of the limit, have a wave count that is no multiple of 4, so that the last workgroup has idle waves.
    Their boxes hold 2^26 cells and more: the reference covers the cells that meet the world, and the rest is compared
    with 0 on the device"""
    vx, torch = eng
    f = 1 << shift
    idle = (shift, dims) in IDLE_WAVES
    S = f ** 3 * dims[0] * dims[1] * dims[2]
    assert (1 << 32) - (1 << 25) < S < 1 << 32 and _reduce_waves(dims, shift) % 4 != 0 if idle else S == 1 << 32
    rng = np.random.default_rng(shift)
    vox = rng.random((256, 256, 256)) < 0.3
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 32))
        assert ctx.lod_workspace_bytes(dims, shift) == (R.workspace_bytes(dims, shift) if idle else 1 << 29)
        o = (-3 * f - 1, -2 * f - 5, -f - 2)
        inside = tuple(-(-(256 - a) // f) for a in o)  # cells that meet the world
        if shift <= 2:
            got, want = _assert_lod_of_the_part_inside(torch, ctx, vox, o, dims, shift, f ** 3 // 4, inside)
            assert all(a < b for a, b in zip(inside, dims))
        else:
            got, want = _assert_lod(ctx, vox, o, dims, shift, f ** 3 // 4, counts=False)
            grid = got.grid()
            assert not grid[inside[0]:].any() and not grid[:, inside[1]:].any() and not grid[:, :, inside[2]:].any()
        assert got.summary.solid == int(vox.sum()) and got.summary.set > 0
    finally:
        ctx.close()


def test_refusals_in_order_leave_the_outputs_untouched(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        ws = ctx.lod_workspace_bytes((8, 8, 8), 2)
        assert ws == 4 * 32 * 32 and ctx.lod_workspace_bytes((8, 8, 8), 0) == 0 and ctx.lod_workspace_bytes((8, 8, 8), 6) == 0
        assert ctx.lod_workspace_bytes((64, 64, 33), 5) == 0 and ctx.lod_workspace_bytes((0, 8, 8), 2) == 0
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        bits = torch.full((4096,), 0x1234, dtype=torch.int32, device="cuda")
        cnt = torch.full((4096,), 0x1234, dtype=torch.int16, device="cuda")
        summ = torch.full((8,), 0x55, dtype=torch.int32, device="cuda")
        hb, hc, hs = np.full(4096, 0x1234, np.uint32), np.full(4096, 0x1234, np.uint16), np.full(8, 0x55, np.uint32)
        i3 = lambda *v: (C.c_int32 * 3)(*v)
        o3, d3 = i3(0, 0, 0), i3(8, 8, 8)

        def call(o=o3, d=d3, sh=2, t=1, wk=work.data_ptr(), b=bits.data_ptr(), c=cnt.data_ptr(), s=summ.data_ptr(), ctxh=h):
            return L.vxrt_downsample_region(ctxh, o, d, sh, t, wk, b, c, s, None)

        def host(o=o3, d=d3, sh=2, t=1, b=hb.ctypes.data, c=hc.ctypes.data, s=hs.ctypes.data):
            return L.vxrt_downsample_region_host(h, o, d, sh, t, b, c, s)

        def why():
            return L.vxrt_last_error().decode()

        def untouched():
            torch.cuda.synchronize()
            dev = bool((bits == 0x1234).all()) and bool((cnt == 0x1234).all()) and bool((summ == 0x55).all())
            return dev and (hb == 0x1234).all() and (hc == 0x1234).all() and (hs == 0x55).all()
        assert call() == -3 and host() == -3 and untouched()    # no world: after every argument check ...
        bad_d, bad_o = i3(8, 0, 8), i3(INT32_MAX - 31, 0, 0)
        # ... which come in the order of the call rules: each call breaks its rule and every later one
        assert call(ctxh=None, o=None, sh=9, t=0, d=bad_d) == -1 and "NULL" in why()
        for k in ("o", "d", "wk", "b", "s"):
            assert call(**{k: None}, sh=9) == -1 and "NULL" in why(), k
        for k in ("o", "d", "b", "s"):
            assert host(**{k: None}, sh=9) == -1 and "NULL" in why(), k
        for sh in (0, 6, 0xFFFFFFFF):
            assert call(sh=sh, t=0, d=bad_d, o=bad_o) == -1 and "lod shift" in why()
            assert host(sh=sh, t=0, d=bad_d, o=bad_o) == -1 and "lod shift" in why()
        for sh, t in [(1, 0), (1, 9), (2, 65), (5, 32769), (3, 0xFFFFFFFF)]:
            assert call(sh=sh, t=t, d=bad_d, o=bad_o) == -1 and "lod threshold" in why(), (sh, t)
            assert host(sh=sh, t=t, d=bad_d, o=bad_o) == -1 and "lod threshold" in why(), (sh, t)
        for sh, bad in [(2, (0, 8, 8)), (2, (8, -1, 8)), (5, (64, 64, 33)), (1, (1024, 1024, 513)), (5, (INT32_MAX, INT32_MAX, INT32_MAX))]:
            assert call(sh=sh, d=i3(*bad), o=bad_o) == -1 and "lod dims" in why(), bad
            assert host(sh=sh, d=i3(*bad), o=bad_o) == -1 and "lod dims" in why(), bad
        for bad in [(INT32_MAX - 31, 0, 0), (0, INT32_MAX - 31, 0), (0, 0, INT32_MAX)]:
            assert call(o=i3(*bad)) == -1 and "lod box: origin" in why(), bad
            assert host(o=i3(*bad)) == -1 and "lod box: origin" in why(), bad
        assert untouched()
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        assert call(sh=0) == -1 and call(t=65) == -1 and call(d=bad_d) == -1 and call(o=bad_o) == -1
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        assert call() == -1 and host() == -1 and "streamed" in why()   # a streamed world
        ctx.stream_close()
        assert untouched()
        ctx.load_world(path)
        # the ends of int32: the least origin, and the last one whose source box fits
        assert call(o=i3(INT32_MIN, INT32_MAX - 32, 0)) == 0
        torch.cuda.synchronize()
        assert _summary(_u32(summ)) == (0, 0, 512, 0, 0, 0) and bool((bits[:8 * 8] == 0).all()) and bool((bits[64:] == 0x1234).all())
        assert call(c=None) == 0 and host(c=None) == 0
        torch.cuda.synchronize()
        assert int(summ[2]) > 0 and bool((cnt[512:] == 0x1234).all()) and (hc == 0x1234).all() and np.array_equal(hs, _u32(summ))
        assert call() == 0 and host() == 0
        torch.cuda.synchronize()
        assert np.array_equal(_u32(bits)[:64], hb[:64]) and np.array_equal(cnt.cpu().numpy().view(np.uint16)[:512], hc[:512])
    finally:
        ctx.close()


def test_headless_example_lod_lines(vxo, tmp_path):
    """examples/voxelapp_headless kind 9 (VoxelRaytracer3D::DownsampleRegion): the printed summary equals the reference's, and
    the hashes of the facade's two vectors equal the hashes of the reference's arrays"""
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    cases = [((-3, 0, -5), (70, 66, 67), 2, 1), ((1, 2, 3), (17, 16, 18), 4, 2048), ((0, 0, 0), (9, 8, 8), 5, 32768)]
    sf = tmp_path / "edits.txt"
    sf.write_text("".join("0 9 %d %d %d %d %d %d %d\n" % (s | t << 3, *o, *d) for o, d, s, t in cases))
    out = subprocess.run([exe, str(edge), "1", str(tmp_path / "dv"), "64", "48", "1", "-", "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [x for x in out.stdout.splitlines() if x.startswith("lod ")]
    expect = []
    for o, d, s, t in cases:
        w = _want(vox, o, d, s, t)
        m = _summary(w.summary)
        expect.append("lod frame 0 shift %d threshold %d set %d empty %d full %d mixed %d max %d solid %d" % (s, t, m[1], m[2], m[3], m[4], m[5], m[0]))
        expect.append("lod hash frame 0 bits %016x counts %016x" % (R.fnv1a(w.words.tobytes()), R.fnv1a(w.flat.tobytes())))
    assert _summary(_want(vox, *cases[0]).summary)[1] > 500
    assert lines == expect, out.stdout
