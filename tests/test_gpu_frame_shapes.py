"""Render launches across strips, checkerboard, AOVs and tall frames, on the device, against the model of
tests/frame_shape_cases.py and the CPU oracle: what each launch writes into each of its buffers (frame, colour AOV, hit AOV,
accumulation history), at which rows, and what it counts.  Every sharded case runs plain and under checkerboard with both
frame parities, for each shard, compact and full-size, on the persistent kernel (its timed and its probe-counting
instantiation) and on k_render (variant 1), whose own copy of the map is tested here only.  Buffers are pre-filled with stale
patterns and have guard rows behind them; everything is bit equality except the colour AOV's finite entries (COLOR_TOL of
tests/test_gpu_parity.py).  The tall and wide frames reach the end of the tile-row schedule, the largest packed
row | view << 16, the refusal above 65535 rows and x / W beyond 16 bits (the 70003-wide frame here and the family of
tests/tools/exact_div_check.c cover that division); the de-interleave cases make k_deinterleave's capped grid loop."""
import numpy as np
import pytest

from tests import frame_shape_cases as FS
from tests import helpers
from tests.test_gpu_parity import COLOR_TOL

pytestmark = pytest.mark.gpu

KERNELS = ((4, False), (4, True), (1, False))  # (variant, collect_stats)
G = FS.GUARD_ROWS


@pytest.fixture(scope="module")
def gpu(vxo):
    import torch
    import voxelengine_amd as vx
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ctx = helpers.new_ctx(vx)
    ctx.SetOrthoWindowSize(10.0, 10.0)   # make_params' default
    helpers.upload(ctx, FS.world(vxo))
    yield vx, ctx, torch
    ctx.close()


def _options(vx, case, mode, shard, compact, stats, frame_number=None, **kw):
    cb, fn = FS.MODES[mode]
    return vx.RenderOptions(checkerboard=bool(cb), frame_number=fn if frame_number is None else frame_number,
                            strip_rows=case.strip_rows, strip_count=case.strip_count, strip_index=shard, compact=compact,
                            collect_stats=stats, shadow=bool(kw.get("shadow", 0)), bounce_samples=kw.get("bounce_samples", 0),
                            bounce_all_hits=bool(kw.get("bounce_all_hits", 0)), ortho=bool(kw.get("ortho", 0)),
                            tile_schedule=kw.get("tile_schedule", True))


def _stale(case, shard, compact, seed=11):
    rows = case.buffer_rows(shard, compact)
    return {"fb": FS.stale_pattern((rows, case.W, 4), np.uint8, seed), "color": FS.stale_pattern((rows, case.W, 3), np.float32, seed + 1),
            "hit": FS.stale_pattern((rows, case.W), np.int64, seed + 2)}


def _launch(gpu, vxo, case, cam, mode, shard, compact, variant, stats, stale=None, tile_order=None, frame_number=None, **kw):
    """one RenderScreen with all three buffers over stale patterns: the buffers as numpy arrays, the counters, the patterns"""
    vx, ctx, torch = gpu
    stale = stale or _stale(case, shard, compact)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in stale.items()}
    pos, f, u, r = helpers.camera(cam, FS.world(vxo).dims, vxo)
    opts = _options(vx, case, mode, shard, compact, stats, frame_number, **kw)
    ctx.set_kernel_variant(variant)
    try:
        assert ctx.kernel_for_launch(case.W, case.H, opts) == (1 if variant == 1 else 7)
        ctx.frame_stats()
        ctx.RenderScreen(case.W, case.H, dev["fb"], pos, f, u, r, opts, color_aov=dev["color"], hit_aov=dev["hit"],
                         tile_order=None if tile_order is None else torch.from_numpy(tile_order.astype(np.int32)).cuda())
        st = ctx.frame_stats()
    finally:
        ctx.set_kernel_variant(4)
    return {k: v.cpu().numpy() for k, v in dev.items()}, st, stale


def _assert_color(got, want, stale, touched, what):
    """the colour AOV: untouched entries bit-equal to the pattern; NaN and infinities exactly where the oracle has them, the
    finite entries within COLOR_TOL"""
    assert np.array_equal(got[~touched].view(np.uint32), stale[~touched].view(np.uint32)), what
    g, w = got[touched], want[touched]
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    assert np.array_equal(np.isposinf(g), np.isposinf(w)) and np.array_equal(np.isneginf(g), np.isneginf(w)), what
    fin = np.isfinite(w)
    assert np.max(np.abs(g[fin] - w[fin]), initial=0.0) <= COLOR_TOL, what


def _assert_buffers(case, full, got, stale, shard, compact, mode, what):
    assert np.array_equal(got["fb"], case.expected_shard(full["fb"], stale["fb"], shard, compact, mode)), what
    assert np.array_equal(got["hit"], case.expected_shard(full["hit"], stale["hit"], shard, compact, mode)), what
    touched = case.expected_shard(np.ones((case.H, case.W), bool), np.zeros(stale["hit"].shape, bool), shard, compact, mode)
    _assert_color(got["color"], case.expected_shard(full["color"], stale["color"], shard, compact, mode), stale["color"], touched, what)


def _assert_counters(st, want, stats, what):
    assert {k: int(getattr(st, k)) for k in FS.RAY_COUNTERS} == {k: want[k] for k in FS.RAY_COUNTERS}, what
    if stats:
        assert {k: int(getattr(st, k)) for k in FS.PROBE_COUNTERS} == {k: want[k] for k in FS.PROBE_COUNTERS}, what
        assert int(st.guard_stray_loads) == 0, what


# ---- the five sharded cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(FS.MODES))
@pytest.mark.parametrize("case", FS.SHARDED, ids=lambda c: c.name)
def test_shard_buffers_and_counters_are_the_models(gpu, vxo, case, mode):
    for cam in ("A", "D"):
        full = FS.oracle_full(vxo, case, cam, mode, **FS.HIT_MIX)
        for shard in range(case.strip_count):
            want = FS.oracle_shard_stats(vxo, case, cam, mode, shard, **FS.HIT_MIX)
            for compact in (True, False):
                for variant, stats in KERNELS:
                    what = (case, cam, mode, shard, compact, variant, stats)
                    got, st, stale = _launch(gpu, vxo, case, cam, mode, shard, compact, variant, stats, **FS.HIT_MIX)
                    _assert_buffers(case, full, got, stale, shard, compact, mode, what)
                    _assert_counters(st, want, stats, what)


@pytest.mark.parametrize("mode", list(FS.MODES))
def test_a_shard_that_owns_nothing_writes_and_counts_nothing(gpu, vxo, mode):
    """shards 2-4 of the 40 x 30 frame: no launch at all when plain, a launch of dead pixels under checkerboard"""
    case = FS.SHARDED_BY_NAME["40x30_16x5"]
    for shard in (2, 3, 4):
        assert case.compact_rows(shard) == 0 and not case.shard_mask(shard, mode).any()
        for compact in (True, False):
            for variant, stats in KERNELS:
                got, st, stale = _launch(gpu, vxo, case, "A", mode, shard, compact, variant, stats, **FS.HIT_MIX)   # returns success
                for k in stale:
                    assert np.array_equal(got[k].view(np.uint8), stale[k].view(np.uint8)), (mode, shard, compact, variant, stats, k)
                assert st.total_rays() == 0 and st.primary_hits == 0
                assert (st.coarse_probes, st.brick_entries, st.fine_probes) == (0, 0, 0)


@pytest.mark.parametrize("mode", list(FS.MODES))
@pytest.mark.parametrize("name", ["72x93_8x3", "40x30_16x5", "64x45_5x2"])
def test_compact_shards_reassemble_to_the_oracles_frame(gpu, vxo, name, mode):
    vx, ctx, torch = gpu
    case = FS.SHARDED_BY_NAME[name]
    assert case.W % 4 == 0
    max_rows = max(case.compact_rows(s) for s in range(case.strip_count)) + G
    shards = FS.stale_pattern((case.strip_count, max_rows, case.W, 4), np.uint8, 21)
    # the background the de-interleaved frame shows where nothing was written: each row's bytes in its owner's buffer
    y = np.arange(case.H)
    background = shards[case.owner(y), case.packed_row(y)]
    want = FS.world(vxo).render(FS.params(vxo, case, "A", mode, **FS.HIT_MIX), fb=background.copy(), nthreads=16)["fb"]
    pos, f, u, r = helpers.camera("A", FS.world(vxo).dims, vxo)
    for variant, stats in KERNELS:
        d_shards = torch.from_numpy(shards.copy()).cuda()
        ctx.set_kernel_variant(variant)
        try:
            for s in range(case.strip_count):
                ctx.RenderScreen(case.W, case.H, d_shards[s], pos, f, u, r, _options(vx, case, mode, s, True, stats, **FS.HIT_MIX))
        finally:
            ctx.set_kernel_variant(4)
        out = torch.full((case.H + G, case.W, 4), 201, dtype=torch.uint8, device="cuda")
        ctx.deinterleave_strips(case.W, case.H, case.strip_rows, case.strip_count, d_shards, max_rows * case.W * 4, out)
        out = out.cpu().numpy()
        assert np.array_equal(out[:case.H], want) and (out[case.H:] == 201).all(), (variant, stats)
    ctx.frame_stats()


@pytest.mark.parametrize("checkerboard", [0, 1])
def test_accumulation_history_of_a_compact_shard(gpu, vxo, checkerboard):
    """d_accum of a compact shard holds the shard's own rows: three frames with a reset at the third; the frame and the
    history, as bits, equal the oracle's full-frame run passed through expected_shard after every frame"""
    vx, ctx, torch = gpu
    case = FS.SHARDED_BY_NAME["72x93_8x3"]
    w = FS.world(vxo)
    pos, f, u, r = helpers.camera("A", w.dims, vxo)
    kw = dict(shadow=1, bounce_samples=1)
    for shard in range(case.strip_count):
        rows = case.buffer_rows(shard, True)
        stale_fb = FS.stale_pattern((rows, case.W, 4), np.uint8, 31)
        stale_acc = FS.stale_pattern((rows, case.W, 4), np.float32, 32)
        stale_acc[:rows - G] = 0.0   # an empty history (frames == 0) with guard rows behind it
        for variant, stats in KERNELS:
            fb_c = case.unpack(stale_fb, shard, True, np.zeros((case.H, case.W, 4), np.uint8))
            acc_c = np.zeros((case.H, case.W, 4), np.float32)
            fb_g, acc_g = torch.from_numpy(stale_fb.copy()).cuda(), torch.from_numpy(stale_acc.copy()).cuda()
            ctx.set_kernel_variant(variant)
            try:
                for frame in (1, 2, 3):
                    p = vxo.make_params(case.W, case.H, pos, f, u, r, frame_number=frame, checkerboard=checkerboard, **kw)
                    w.render(p, fb=fb_c, accum=acc_c, accum_reset=frame == 3, nthreads=16)
                    opts = _options(vx, case, "checker_odd" if checkerboard else "plain", shard, True, stats, frame_number=frame, **kw)
                    ctx.RenderScreen(case.W, case.H, fb_g, pos, f, u, r, opts, accum=acc_g, accum_reset=frame == 3)
                    what = (checkerboard, shard, variant, stats, frame)
                    # (every row of the shard: both sides keep what earlier frames wrote)
                    assert np.array_equal(fb_g.cpu().numpy(), case.expected_shard(fb_c, stale_fb, shard, True, "plain")), what
                    assert np.array_equal(acc_g.cpu().numpy().view(np.uint32),
                                          case.expected_shard(acc_c, stale_acc, shard, True, "plain").view(np.uint32)), what
                    assert (acc_c[case.rows_of(shard)][..., 3] > 0).any()
            finally:
                ctx.set_kernel_variant(4)
    ctx.frame_stats()


@pytest.mark.parametrize("checkerboard", [0, 1])
@pytest.mark.parametrize("name", ["72x93_8x3", "61x92_12x4"])
def test_multi_view_shards_are_the_models(gpu, vxo, name, checkerboard):
    """three views (cameras A, D, B; frame numbers of mixed parity) in one launch, each with its own compact AOVs: every view
    against the model's expectation, not merely against the single-view launch"""
    vx, ctx, torch = gpu
    case = FS.SHARDED_BY_NAME[name]
    cams, frames = ("A", "D", "B"), (3, 4, 7)
    modes = [("checker_even" if fn % 2 == 0 else "checker_odd") if checkerboard else "plain" for fn in frames]
    fulls = [FS.oracle_full(vxo, case, cam, mode, frame_number=fn, **FS.HIT_MIX) for cam, mode, fn in zip(cams, modes, frames)]
    for shard in range(case.strip_count):
        for variant, stats in KERNELS:
            stales = [_stale(case, shard, True, seed=40 + 3 * j) for j in range(3)]
            dev = [{k: torch.from_numpy(v.copy()).cuda() for k, v in s.items()} for s in stales]
            views = []
            for cam, fn, d in zip(cams, frames, dev):
                pos, f, u, r = helpers.camera(cam, FS.world(vxo).dims, vxo)
                views.append(dict(fb=d["fb"], origin=pos, fwd=f, up=u, right=r, frame_number=fn, color_aov=d["color"], hit_aov=d["hit"]))
            opts = _options(vx, case, modes[0], shard, True, stats, **FS.HIT_MIX)
            ctx.set_kernel_variant(variant)
            try:
                assert ctx.kernel_for_launch(case.W, case.H, opts, nviews=3) == (1 if variant == 1 else 7)
                ctx.frame_stats()
                ctx.RenderViews(case.W, case.H, views, opts)
                st = ctx.frame_stats()
            finally:
                ctx.set_kernel_variant(4)
            want = dict.fromkeys(FS.RAY_COUNTERS + FS.PROBE_COUNTERS, 0)
            for cam, mode, fn, full, d, stale in zip(cams, modes, frames, fulls, dev, stales):
                got = {k: v.cpu().numpy() for k, v in d.items()}
                _assert_buffers(case, full, got, stale, shard, True, mode, (case, shard, variant, stats, cam))
                one = FS.oracle_shard_stats(vxo, case, cam, mode, shard, frame_number=fn, **FS.HIT_MIX)
                for k in want:
                    want[k] += one[k]
            _assert_counters(st, want, stats, (case, shard, variant, stats))


def test_the_callers_tile_order_never_changes_a_sharded_or_checkerboard_launch(gpu, vxo):
    """d_tile_order is a permutation of the LAUNCH grid's tiles: ceil(W/8) * ceil(compact_rows/8) for a plain compact shard,
    ceil(W/8) * ceil((H >> 1)/8) under checkerboard"""
    rng = np.random.default_rng(5)
    for name, mode in (("72x93_8x3", "plain"), ("61x92_12x4", "checker_even"), ("61x92_12x4", "checker_odd")):
        case = FS.SHARDED_BY_NAME[name]
        full = FS.oracle_full(vxo, case, "A", mode, **FS.HIT_MIX)
        for shard in range(case.strip_count):
            ntiles = FS.ceil_div(case.W, 8) * FS.ceil_div(case.launch_rows(shard, FS.MODES[mode][0]), 8)
            assert ntiles > 8
            for stats in (False, True):
                got, st, stale = _launch(gpu, vxo, case, "A", mode, shard, True, 4, stats, tile_order=rng.permutation(ntiles), **FS.HIT_MIX)
                _assert_buffers(case, full, got, stale, shard, True, mode, (name, mode, shard, stats))
                _assert_counters(st, FS.oracle_shard_stats(vxo, case, "A", mode, shard, **FS.HIT_MIX), stats, (name, mode, shard))


# ---- tall and wide frames --------------------------------------------------------------------------------------------------
def _assert_unsharded(gpu, vxo, case, cam, mode, kernels=((4, False), (1, False)), **kw):
    full = FS.oracle_full(vxo, case, cam, mode, **{k: v for k, v in kw.items() if k != "tile_schedule"})   # (scheduling only)
    for variant, stats in kernels:
        got, st, stale = _launch(gpu, vxo, case, cam, mode, 0, False, variant, stats, **kw)
        what = (case, cam, mode, variant, kw)
        _assert_buffers(case, full, got, stale, 0, False, mode, what)
        assert st.primary_rays == full["stats"].primary_rays == int(case.shard_mask(0, mode).sum()), what
        assert st.primary_hits == full["stats"].primary_hits and st.shadow_rays == full["stats"].shadow_rays, what


@pytest.mark.parametrize("tile_schedule", [True, False])
@pytest.mark.parametrize("case", [FS.TALL_ON, FS.TALL_OFF], ids=lambda c: c.name)
def test_frames_either_side_of_the_tile_row_schedules_cap(gpu, vxo, case, tile_schedule):
    """512 and 513 tile rows (that the first takes a schedule and the second none is the host test's restated nty <= cap):
    the frames equal the oracle's with the schedule asked for and not"""
    _assert_unsharded(gpu, vxo, case, "A", "plain", shadow=1, tile_schedule=tile_schedule)
    _assert_unsharded(gpu, vxo, case, "D", "checker_even", kernels=((4, False),), tile_schedule=tile_schedule)


@pytest.mark.parametrize("mode", ["plain", "checker_odd"])
def test_the_tallest_frame(gpu, vxo, mode):
    full = FS.oracle_full(vxo, FS.TALLEST, "A", mode, shadow=1)
    assert 0 < full["stats"].primary_hits < full["stats"].primary_rays
    _assert_unsharded(gpu, vxo, FS.TALLEST, "A", mode, shadow=1)


@pytest.mark.parametrize("checkerboard", [0, 1])
def test_two_views_of_the_tallest_frame(gpu, vxo, checkerboard):
    """rows 65528 .. 65534 live in the last tile row of view 1, where the packed row | view << 16 is largest"""
    vx, ctx, torch = gpu
    case = FS.TALLEST
    cams, frames = ("A", "D"), (3, 4)
    modes = [("checker_even" if fn % 2 == 0 else "checker_odd") if checkerboard else "plain" for fn in frames]
    fulls = [FS.oracle_full(vxo, case, cam, mode, frame_number=fn, shadow=1) for cam, mode, fn in zip(cams, modes, frames)]
    for variant in (4, 1):
        stales = [_stale(case, 0, False, seed=60 + 3 * j) for j in range(2)]
        dev = [{k: torch.from_numpy(s[k].copy()).cuda() for k in ("fb", "hit")} for s in stales]
        views = []
        for cam, fn, d in zip(cams, frames, dev):
            pos, f, u, r = helpers.camera(cam, FS.world(vxo).dims, vxo)
            views.append(dict(fb=d["fb"], origin=pos, fwd=f, up=u, right=r, frame_number=fn, hit_aov=d["hit"]))
        opts = _options(vx, case, modes[0], 0, False, False, shadow=1)
        ctx.set_kernel_variant(variant)
        try:
            assert ctx.kernel_for_launch(case.W, case.H, opts, nviews=2) == (1 if variant == 1 else 7)
            ctx.frame_stats()
            ctx.RenderViews(case.W, case.H, views, opts)
            st = ctx.frame_stats()
        finally:
            ctx.set_kernel_variant(4)
        for mode, full, d, stale in zip(modes, fulls, dev, stales):
            for k in ("fb", "hit"):
                assert np.array_equal(d[k].cpu().numpy(), case.expected_shard(full[k], stale[k], 0, False, mode)), (variant, mode, k)
        assert st.primary_rays == sum(f["stats"].primary_rays for f in fulls)
        assert st.primary_hits == sum(f["stats"].primary_hits for f in fulls) == st.shadow_rays


def test_the_tallest_frame_in_compact_shards(gpu, vxo):
    case = FS.TALLEST_SHARDED
    full = FS.oracle_full(vxo, FS.TALLEST, "A", "plain", shadow=1)
    for shard in range(case.strip_count):
        m = case.shard_mask(shard, "plain")
        hits = int((full["hit"][m] >= 0).sum())
        for variant in (4, 1):
            got, st, stale = _launch(gpu, vxo, case, "A", "plain", shard, True, variant, False, shadow=1)
            _assert_buffers(case, full, got, stale, shard, True, "plain", (shard, variant))
            assert (st.primary_rays, st.primary_hits, st.shadow_rays, st.bounce_rays) == (int(m.sum()), hits, hits, 0)


@pytest.mark.parametrize("ortho", [0, 1])
def test_a_frame_wider_than_sixteen_bits(gpu, vxo, ortho):
    """x / W with W = 70003, beyond the 16-bit family of tests/test_exact_division.py (which also walks this width).
    Perspective: camera A, whose sky gradient and colour AOV vary with x; ortho: camera C looking down through a window as wide
    as the world, so that the origins x / W places see hits and misses."""
    vx, ctx, torch = gpu
    if not ortho:
        _assert_unsharded(gpu, vxo, FS.WIDE, "A", "plain", shadow=1)
        return
    window = (0.004, 30.0)
    full = FS.oracle_full(vxo, FS.WIDE, "C", "plain", shadow=1, ortho=1, ortho_size=window)
    assert 1000 < full["stats"].primary_hits < full["stats"].primary_rays - 1000 and len(np.unique(full["hit"])) > 100
    ctx.SetOrthoWindowSize(*window)
    try:
        _assert_unsharded(gpu, vxo, FS.WIDE, "C", "plain", shadow=1, ortho=1, ortho_size=window)
    finally:
        ctx.SetOrthoWindowSize(10.0, 10.0)


def test_refused_launches_leave_buffers_and_counters_untouched(gpu, vxo):
    """65536 rows (one view and sixteen), and bad strip arguments with strip_count > 1: VXRT_ERR_INVALID, nothing written"""
    vx, ctx, torch = gpu
    caps = FS.read_caps()
    pos, f, u, r = helpers.camera("A", FS.world(vxo).dims, vxo)
    small = FS.SHARDED_BY_NAME["72x93_8x3"]
    refused = [(FS.TOO_TALL, dict(), 1), (FS.TOO_TALL, dict(), caps["max_views"]),
               (small, dict(strip_rows=8, strip_count=3, strip_index=3), 1), (small, dict(strip_rows=8, strip_count=3, strip_index=-1), 1),
               (small, dict(strip_rows=0, strip_count=3, strip_index=1), 1)]
    for case, strips, nviews in refused:
        stale = {"fb": FS.stale_pattern((case.H, case.W, 4), np.uint8, 71), "color": FS.stale_pattern((case.H, case.W, 3), np.float32, 72),
                 "hit": FS.stale_pattern((case.H, case.W), np.int64, 73)}
        dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in stale.items()}
        opts = vx.RenderOptions(shadow=True, frame_number=3, **strips)
        for variant in (4, 1):
            ctx.set_kernel_variant(variant)
            try:
                ctx.frame_stats()
                with pytest.raises(vx.VxrtError, match=r"vxrt error -1:"):   # VXRT_ERR_INVALID
                    if nviews == 1:
                        ctx.RenderScreen(case.W, case.H, dev["fb"], pos, f, u, r, opts, color_aov=dev["color"], hit_aov=dev["hit"])
                    else:
                        ctx.RenderViews(case.W, case.H, [dict(fb=dev["fb"], origin=pos, fwd=f, up=u, right=r, frame_number=3,
                                                              color_aov=dev["color"], hit_aov=dev["hit"])] * nviews, opts)
                st = ctx.frame_stats()
            finally:
                ctx.set_kernel_variant(4)
            assert st.total_rays() == 0 and st.primary_hits == 0, (case, strips, nviews, variant)
            for k in stale:
                assert np.array_equal(dev[k].cpu().numpy().view(np.uint8), stale[k].view(np.uint8)), (case, strips, nviews, variant, k)


# ---- k_deinterleave past its grid cap ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FS.DEINTERLEAVE, ids=lambda c: c.name)
def test_deinterleave_beyond_its_grid_cap(gpu, case):
    """563 200 lanes of 16 bytes for at most 2048 x 256 threads: the kernel's grid-stride loop repeats.  Random shard bytes
    against a numpy gather built from the model's owner and packed_row, one view and two."""
    vx, ctx, torch = gpu
    caps = FS.read_caps()
    assert case.W // 4 * case.H > caps["deinterleave_blocks"] * caps["deinterleave_threads"]
    views = 2
    max_rows = max(case.compact_rows(s) for s in range(case.strip_count))
    shard_bytes = max_rows * case.W * 4
    shards = np.random.default_rng(9).integers(0, 256, size=(case.strip_count, views, max_rows, case.W, 4), dtype=np.uint8)
    y = np.arange(case.H)
    want = np.stack([shards[case.owner(y), j, case.packed_row(y)] for j in range(views)])
    d_shards = torch.from_numpy(shards).cuda()
    one = torch.full((case.H + G, case.W, 4), 201, dtype=torch.uint8, device="cuda")
    ctx.deinterleave_strips(case.W, case.H, case.strip_rows, case.strip_count, d_shards, views * shard_bytes, one)
    one = one.cpu().numpy()
    assert np.array_equal(one[:case.H], want[0]) and (one[case.H:] == 201).all()
    both = torch.full((views, case.H + G, case.W, 4), 201, dtype=torch.uint8, device="cuda")
    ctx.deinterleave_views(case.W, case.H, case.strip_rows, case.strip_count, d_shards, views * shard_bytes, shard_bytes, views, both,
                           (case.H + G) * case.W * 4)
    both = both.cpu().numpy()
    assert np.array_equal(both[:, :case.H], want) and (both[:, case.H:] == 201).all()
