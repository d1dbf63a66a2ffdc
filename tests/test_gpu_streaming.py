"""Chunk streaming on the GPU (include/vxrt.h, vxrt_stream_*) against the model of its policy (tests/ref_stream.py,
StreamModelA): after every focus call of random sequences on four worlds -- factor 8 with chunks left empty, factor 16 and
32 terrain on grids whose chunk counts differ on every axis, and a wide grid (129 chunks along x, cx > 1020) flown along x
with a small pool -- the eight stats, the flags and vxrt_download_world (coarse bits, slots, bounds and the whole pool,
stale bricks included) equal the model's cache; at three points of each sequence frames of the persistent (7, timed and
probe-counting) and cross-check (1) kernels, a 4-view launch and a ray batch equal the oracle on the world truncated to the
resident chunks.  Then the refused calls (each leaves the world as it was), the transitions between streamed, uploaded and
no world, a saved cache loaded elsewhere, a file cut short under an open stream, and the ordering of launches on a side
stream around a focus call."""
import os

import numpy as np
import pytest

from tests import helpers
from tests import ref_stream as R
from tests.test_gpu_parity import _assert_batch_equal, _assert_frame_equal, _render_both, eng  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = 64, 48
HEADER_BYTES = 120
_WORLDS = {}


def world(vxo, name):
    """(oracle World, dense voxels or None)"""
    if name not in _WORLDS:
        if name == "random8":            # 2 x 1 x 3 chunks of 64^3 voxels; chunks 1 and 2 empty, chunk 4 nearly so
            rng = np.random.default_rng(8)
            v = rng.random((128, 64, 192)) < 0.002
            v[64:128, :, 0:64] = False
            v[0:64, :, 64:128] = False
            v[64:128, :, 128:192] &= rng.random((64, 64, 64)) < 0.1
            _WORLDS[name] = (vxo.World.from_voxels(v, 8), v)
        elif name == "terrain16":        # 3 x 2 x 5 chunks
            _WORLDS[name] = (vxo.World.generate(vxo.GEN_INT_TERRAIN, 384, 256, 640, 16, nthreads=16), None)
        elif name == "terrain32":        # 2 x 1 x 3 chunks
            _WORLDS[name] = (vxo.World.generate(vxo.GEN_INT_TERRAIN, 512, 256, 768, 32, nthreads=16), None)
        elif name == "wide8":            # 129 x 1 x 1 chunks: cx = 1032
            rng = np.random.default_rng(129)
            v = np.zeros((129 * 64, 64, 64), bool)
            n = 4000
            v[rng.integers(0, v.shape[0], n), rng.integers(0, 64, n), rng.integers(0, 64, n)] = True
            v[:, 0, :] = True
            _WORLDS[name] = (vxo.World.from_voxels(v, 8), v)
        else:
            raise KeyError(name)
    return _WORLDS[name]


@pytest.fixture(scope="module")
def files(eng, vxo, tmp_path_factory):
    """name -> the world's brickmap file (written by vxrt_save_world from an uploaded world)"""
    vx, _, _ = eng
    d = tmp_path_factory.mktemp("streamed")
    made = {}

    def get(name):
        if name not in made:
            w, _ = world(vxo, name)
            c = vx.Context(0)
            try:
                helpers.upload(c, w)
                c.save_world(str(d / (name + ".vxb")))
            finally:
                c.close()
            made[name] = str(d / (name + ".vxb"))
        return made[name]
    return get


def stats_tuple(st):
    return tuple(int(getattr(st, f)) for f in R.STAT_FIELDS)


def focus_both(ctx, model, focus, radius, what=""):
    """one focus call on the library and the model, stats and flags asserted equal"""
    want = model.focus(focus, radius)
    assert want["rc"] == R.OK
    st = ctx.stream_focus(focus, radius)
    assert stats_tuple(st) == want["stats"], (what, focus, radius)
    assert np.array_equal(ctx.stream_resident(), want["flags"]), (what, focus, radius)
    return want


def assert_cache(ctx, w, model):
    d = ctx.download_world()
    exp = R.expected_cache(w, model)
    assert np.array_equal(d["coarse_bits"], exp["coarse_bits"])
    assert np.array_equal(d["brick_slot"], exp["brick_slot"])
    assert np.array_equal(d["bounds"].reshape(-1, 6).view(np.uint32), exp["bounds"].view(np.uint32))
    assert np.array_equal(d["pool"], exp["pool"])
    return d


def near_camera(focus, dims, j):
    """a camera above the focus (clamped into the world's x / z span), looking down and along"""
    vxm = __import__("voxelengine_amd")
    pos = (float(F32(min(max(focus[0], 0.0), dims[0]))), float(F32(0.9 * dims[1])), float(F32(min(max(focus[2], 0.0), dims[2]))))
    f, u, r = vxm.GetDirections((-0.5, 0.7 + 0.9 * j, 0.0))
    return (pos, tuple(f), tuple(u), tuple(r))


def assert_frames(eng, vxo, tw, focus, j):
    """frames of kernels 7 (timed and counting) and 1, a 4-view launch and a ray batch against the oracle on `tw`"""
    vx, ctx, torch = eng
    default = ctx.kernel_variant
    cam = near_camera(focus, tw.dims, j)
    try:
        for variant in (7, 1):
            ctx.set_kernel_variant(variant)
            cpu, fb, col, hit, st = _render_both(eng, vxo, tw, W, H, cam, frame_number=j, shadow=1, bounce_samples=1)
            _assert_frame_equal(cpu, fb, col, hit, st)
    finally:
        ctx.set_kernel_variant(default)
    cams = [near_camera(focus, tw.dims, j + k) for k in range(3)] + [helpers.camera("A", tw.dims, vxo)]
    views, wants, rays = [], [], 0
    fb0 = np.random.default_rng(j).integers(0, 255, size=(H, W, 4), dtype=np.uint8)
    for k, c in enumerate(cams):
        p = vxo.make_params(W, H, *c, frame_number=10 + k, shadow=1, bounce_samples=1)
        want = tw.render(p, fb=fb0.copy(), want_hit=True, nthreads=16)
        wants.append(want)
        rays += want["stats"].total_rays()
        views.append(dict(fb=torch.from_numpy(fb0.copy()).cuda(), origin=c[0], fwd=c[1], up=c[2], right=c[3],
                          frame_number=10 + k, hit_aov=torch.full((H, W), -7, dtype=torch.int64, device="cuda")))
    ctx.frame_stats()
    ctx.RenderViews(W, H, views, vx.RenderOptions(shadow=True, bounce_samples=1))
    assert ctx.frame_stats().total_rays() == rays
    for k, (v, want) in enumerate(zip(views, wants)):
        assert np.array_equal(v["fb"].cpu().numpy(), want["fb"]), k
        assert np.array_equal(v["hit_aov"].cpu().numpy(), want["hit"]), k
    o, d = helpers.mixed_rays(tw.dims, 3000, seed=j)
    _assert_batch_equal(ctx.Raytrace(o, d), tw.trace_batch(o, d, nthreads=16))
    return sum(w["stats"].primary_hits for w in wants)


def focus_sequence(rng, t, name, n=25):
    e = 8.0 * t.factor
    ext = np.array(t.cdims, np.float64) * t.factor
    calls = []
    for j in range(n):
        if name == "wide8":              # along x and back, a few chunks' reach
            s = j / (n - 1)
            x = ext[0] * (2 * s if s <= 0.5 else 2 - 2 * s) * 0.97 + rng.uniform(0, 0.03) * ext[0]
            focus = (x, rng.uniform(0, ext[1]), rng.uniform(0, ext[2]))
            radius = rng.uniform(0.5, 3.0) * e
        else:
            if rng.random() < 0.3:       # on chunk faces and centres
                focus = tuple(np.round(rng.uniform(-0.3, 1.3, 3) * ext / (e / 2)) * (e / 2))
            else:
                focus = tuple(rng.uniform(-0.2, 1.2, 3) * ext)
            u = rng.random()
            radius = 0.0 if u < 0.1 else (float("inf") if u < 0.14 else rng.uniform(0.2, 1.6) * e)
        calls.append(([float(F32(c)) for c in focus], float(F32(radius))))
    return calls


def capacities(t, name):
    if name == "wide8":                  # room for five chunks, and for two (chunks within the radius go missing)
        return [int(t.nbricks.max()) * 5 + 3, int(t.nbricks.max()) * 2]
    return [int(t.nbricks.max()) + t.nslots // 10, t.nslots // 2 + 1, t.nslots]   # one big chunk, half, everything


@pytest.mark.parametrize("name", ["random8", "terrain16", "terrain32", "wide8"])
def test_focus_sequences_equal_the_model(eng, vxo, files, name):
    vx, ctx, torch = eng
    w, _ = world(vxo, name)
    t = R.Tables.of(w)
    assert t.nchunks == int(np.prod(w.cdims)) // 512 and (t.nbricks == 0).any() == (name == "random8")
    rng = np.random.default_rng(len(name) * 7 + t.factor)
    seen = dict(evicted=0, missing=0, hits=0)
    for ci, cap in enumerate(capacities(t, name)):
        info = ctx.stream_open(files(name), cap)
        assert (info.factor, tuple(info.cdims), info.nslots) == (w.factor, tuple(w.cdims), cap)
        model = R.StreamModelA(t, cap)
        calls = focus_sequence(rng, t, name)
        for j, (focus, radius) in enumerate(calls):
            want = focus_both(ctx, model, focus, radius, (name, cap, j))
            seen["evicted"] += want["stats"][5]
            seen["missing"] += want["stats"][6]
            assert_cache(ctx, w, model)
            if j in (4, 13, 24):
                seen["hits"] += assert_frames(eng, vxo, R.truncated_world(vxo, w, want["flags"]), focus, 100 * ci + j)
    ctx.stream_close()
    assert seen["evicted"] > 0 and seen["hits"] > 0 and seen["missing"] > 0


def snapshot(eng, vxo):
    vx, ctx, torch = eng
    d = ctx.download_world()
    pos, f, u, r = helpers.camera("A", tuple(c * d["factor"] for c in d["cdims"]), vxo)
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.RenderScreen(W, H, fb, pos, f, u, r, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=1))
    return d, fb.cpu().numpy()


def assert_same(a, b):
    (da, fa), (db, fb) = a, b
    for k in ("coarse_bits", "brick_slot", "pool"):
        assert np.array_equal(da[k], db[k]), k
    assert np.array_equal(da["bounds"].view(np.uint32), db["bounds"].view(np.uint32))
    assert np.array_equal(fa, fb)


def test_refused_calls_leave_the_streamed_world_as_it_was(eng, vxo, files, tmp_path):
    vx, ctx, torch = eng
    w, _ = world(vxo, "terrain32")
    t = R.Tables.of(w)
    path = files("terrain32")
    occ = np.flatnonzero(t.nbricks > 0)
    model = R.StreamModelA(t, t.nslots)
    ctx.stream_open(path, t.nslots)
    # the last occupied chunk first, then the first: the cache's slots are not in cell order
    for ch in (occ[-1], occ[0]):
        focus_both(ctx, model, [float(v) for v in (t.lo[ch] + t.hi[ch]) / 2], 0.0)
    assert sorted(np.flatnonzero(model.flags())) == sorted([occ[0], occ[-1]])
    before = snapshot(eng, vxo)
    nan, inf = float("nan"), float("inf")
    for focus, radius in (((nan, 0.0, 0.0), 10.0), ((0.0, inf, 0.0), 10.0), ((0.0, 0.0, -inf), inf), ((1.0, 2.0, 3.0), -1.0),
                          ((1.0, 2.0, 3.0), nan), ((1.0, 2.0, 3.0), -inf)):
        with pytest.raises(vx.VxrtError, match="error -1"):
            ctx.stream_focus(focus, radius)
        assert_same(snapshot(eng, vxo), before)
    for n in (t.nchunks - 1, t.nchunks + 1, 0):
        with pytest.raises(vx.VxrtError, match="error -1"):
            ctx.stream_resident(n)
    assert np.array_equal(ctx.stream_resident(t.nchunks), model.flags())
    cache = str(tmp_path / "cache.vxb")
    ctx.save_world(cache)
    raw = bytearray(open(path, "rb").read())
    raw[HEADER_BYTES + len(w.coarse_bits) * 4 + 4] ^= 1          # cell 0's extents: the sum of the cell table fails
    corrupt = str(tmp_path / "corrupt.vxb")
    open(corrupt, "wb").write(bytes(raw))
    for p, cap, msg in ((str(tmp_path / "missing.vxb"), 10, "cannot open"), (corrupt, 10, "checksum"),
                        (cache, t.nslots, "cell order"), (path, 0, "empty pool"), (path, 1 << 32, "0xFFFFFFFF"),
                        (path, (1 << 64) - 1, "0xFFFFFFFF")):
        with pytest.raises(vx.VxrtError, match=msg):
            ctx.stream_open(p, cap)
        assert_same(snapshot(eng, vxo), before)
        assert np.array_equal(ctx.stream_resident(), model.flags())
    # the stream itself is untouched: the next call continues the model's sequence
    focus_both(ctx, model, [float(v) for v in (t.lo[occ[1]] + t.hi[occ[1]]) / 2], 0.0)
    assert_cache(ctx, w, model)
    ctx.stream_close()


def test_transitions_between_streamed_uploaded_and_no_world(eng, vxo, files, tmp_path):
    vx, ctx, torch = eng
    w32, _ = world(vxo, "terrain32")
    w8, v8 = world(vxo, "random8")
    t32, t8 = R.Tables.of(w32), R.Tables.of(w8)
    ctx.stream_open(files("terrain32"), t32.nslots // 3)
    m32 = R.StreamModelA(t32, t32.nslots // 3)
    evicted = 0
    for focus, radius in (((100.0, 200.0, 100.0), 300.0), ((500.0, 100.0, 700.0), 300.0), ((0.0, 0.0, 0.0), 200.0)):
        evicted += focus_both(ctx, m32, focus, radius)["stats"][5]
    assert evicted > 0 and 0 < m32.flags().sum() < (t32.nbricks > 0).sum()
    # a saved partly resident cache (after evictions) loads elsewhere: tables equal the download, frames the oracle's
    d = assert_cache(ctx, w32, m32)
    cache = str(tmp_path / "cache.vxb")
    ctx.save_world(cache)
    other = vx.Context(0)
    try:
        other.load_world(cache)
        e = other.download_world()
        for k in ("coarse_bits", "brick_slot", "pool"):
            assert np.array_equal(e[k], d[k]), k
        assert np.array_equal(e["bounds"].view(np.uint32), d["bounds"].view(np.uint32))
        tw = R.truncated_world(vxo, w32, m32.flags())
        for cam in ("A", "D"):
            cpu, fb, col, hit, st = _render_both((vx, other, torch), vxo, tw, W, H, cam, frame_number=2, shadow=1,
                                                 bounce_samples=1)
            _assert_frame_equal(cpu, fb, col, hit, st)
    finally:
        other.close()
    # a second file on the same context: a new, empty cache of the new world
    ctx.stream_open(files("random8"), t8.nslots)
    m8 = R.StreamModelA(t8, t8.nslots)
    assert ctx.stream_resident().sum() == 0 and ctx.world_info().factor == 8
    focus_both(ctx, m8, (64.0, 32.0, 96.0), 40.0)
    assert_cache(ctx, w8, m8)
    # upload_world replaces the streamed world: streaming calls see none, edits work
    helpers.upload(ctx, w8)
    with pytest.raises(vx.VxrtError, match="error -3"):
        ctx.stream_focus((0.0, 0.0, 0.0), 10.0)
    with pytest.raises(vx.VxrtError, match="error -3"):
        ctx.stream_resident()
    ctx.stream_close()                            # nothing to close: not an error, and the uploaded world stays
    ctx.edit_voxels([vx.EditBox((10, 5, 20), (70, 30, 100), 1)])
    v = v8.copy()
    v[10:71, 5:31, 20:101] = True
    helpers.assert_tables(ctx, vxo.World.from_voxels(v, 8))
    # stream_close of a streamed world leaves no world: render and batch refuse
    ctx.stream_open(files("random8"), 10)
    ctx.stream_close()
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    pos, f, u, r = helpers.camera("A", w8.dims, vxo)
    with pytest.raises(vx.VxrtError, match="error -3"):
        ctx.RenderScreen(W, H, fb, pos, f, u, r, vx.RenderOptions())
    with pytest.raises(vx.VxrtError, match="error -3"):
        ctx.Raytrace(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))


def test_a_file_cut_short_fails_at_the_first_unreadable_chunk(eng, vxo, files, tmp_path):
    """A focus call whose order reaches a chunk past the end of a file cut short under the open stream: the loads and
    evictions before that chunk stay, the chunk is not resident, the call fails; a launch on a non-blocking stream straight
    after it sees what the call left; a later call that reaches only readable chunks loads from the cut file."""
    vx, ctx, torch = eng
    w, _ = world(vxo, "terrain16")
    t = R.Tables.of(w)
    path = str(tmp_path / "short.vxb")
    open(path, "wb").write(open(files("terrain16"), "rb").read())
    pool_off = HEADER_BYTES + len(w.coarse_bits) * 4 + w.brick_slot.size * 8
    near, far = [float(v) for v in t.lo[0]], [float(v) for v in t.hi[-1]]
    occupied = t.nbricks > 0
    order = np.argsort(t.d2(near), kind="stable")
    order = order[occupied[order]]
    # the cut: inside the run of the first chunk of the near corner's order that comes after only lower-numbered chunks
    # (slots run in chunk order, so the chunks before it in the order are readable), at least 5 chunks into the order
    k = next(k for k in range(5, order.size) if order[:k].max() < order[k])
    cut_chunk = int(order[k])
    radius = float(F32(np.sqrt(np.float64(t.d2(near)[cut_chunk])) * 1.0001))
    assert F32(radius) * F32(radius) >= t.d2(near)[cut_chunk]
    cap = int(t.nbricks[order[:k]].sum()) + int(t.nbricks.max())    # the chunks before the cut, and one more big one
    ctx.stream_open(path, cap)
    model = R.StreamModelA(t, cap)
    # while the file is whole: chunks of the far corner -- the ones the failing call will have to evict
    first = focus_both(ctx, model, far, 1.5 * 8 * t.factor)
    assert first["stats"][4] >= 3
    cut = pool_off + int(t.first_slot[cut_chunk]) * t.brick_bytes + t.brick_bytes // 2
    os.truncate(path, cut)
    unreadable = {int(c) for c in np.flatnonzero(occupied) if pool_off + int(t.first_slot[c] + t.nbricks[c]) * t.brick_bytes > cut}
    assert unreadable == {int(c) for c in np.flatnonzero(occupied) if c >= cut_chunk}
    want = model.focus(near, radius, unreadable)
    assert want["rc"] == R.READ_FAILED
    loaded = (first["base"] < 0) & (want["base"] >= 0)
    evicted = (first["base"] >= 0) & (want["base"] < 0)
    assert loaded.sum() == k and set(np.flatnonzero(loaded)) == set(order[:k].tolist()) and evicted.sum() > 0
    assert want["base"][cut_chunk] < 0
    with pytest.raises(vx.VxrtError, match="chunk read failed"):
        ctx.stream_focus(near, radius)
    # straight after the failed call, a launch on a non-blocking stream sees the tables and bricks the call left
    side = torch.cuda.Stream()
    cam = near_camera(near, w.dims, 3)           # (cameras 3, 4 and 5 of the near corner look into the loaded chunks)
    tw = R.truncated_world(vxo, w, want["flags"])
    fb = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.RenderScreen(W, H, fb, *cam, vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=4), stream=side.cuda_stream)
    side.synchronize()
    p = vxo.make_params(W, H, *cam, frame_number=4, shadow=1, bounce_samples=1)
    want_fb = tw.render(p, fb=np.zeros((H, W, 4), np.uint8), want_hit=True, nthreads=16)
    assert want_fb["stats"].primary_hits > 0
    assert np.array_equal(fb.cpu().numpy(), want_fb["fb"])
    assert np.array_equal(ctx.stream_resident(), want["flags"])
    assert_cache(ctx, w, model)
    assert_frames(eng, vxo, tw, near, 3)
    # a later focus that reaches only readable chunks -- one the failing call did not get to -- loads from the cut file
    later = next(int(c) for c in np.flatnonzero(occupied) if c < cut_chunk and want["base"][c] < 0)
    centre = [float(v) for v in (t.lo[later] + t.hi[later]) / 2]
    ok = model.focus(centre, 0.0, unreadable)
    assert ok["rc"] == R.OK and ok["stats"][4] == 1
    st = ctx.stream_focus(centre, 0.0)
    assert stats_tuple(st) == ok["stats"] and np.array_equal(ctx.stream_resident(), ok["flags"])
    assert_cache(ctx, w, model)
    ctx.stream_close()


def test_launches_on_a_side_stream_see_the_cache_of_their_turn(eng, vxo, files):
    """a render queued on a non-blocking stream before a focus call draws the old cache, one queued after it the new"""
    vx, ctx, torch = eng
    w, _ = world(vxo, "terrain16")
    t = R.Tables.of(w)
    cap = t.nslots // 3
    ctx.stream_open(files("terrain16"), cap)
    model = R.StreamModelA(t, cap)
    a = focus_both(ctx, model, (64.0, 128.0, 64.0), 200.0)
    flags_a = a["flags"]
    b_focus = (320.0, 128.0, 600.0)
    side = torch.cuda.Stream()
    W2, H2 = 320, 240
    pos, f, u, r = helpers.camera("A", w.dims, vxo)
    opts = vx.RenderOptions(shadow=True, bounce_samples=2, frame_number=9)
    fbs = [torch.zeros((H2, W2, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    ctx.RenderScreen(W2, H2, fbs[0], pos, f, u, r, opts, stream=side.cuda_stream)
    b = focus_both(ctx, model, b_focus, 250.0)
    ctx.RenderScreen(W2, H2, fbs[1], pos, f, u, r, opts, stream=side.cuda_stream)
    side.synchronize()
    assert not np.array_equal(flags_a, b["flags"]) and b["stats"][5] > 0
    p = vxo.make_params(W2, H2, pos, f, u, r, frame_number=9, shadow=1, bounce_samples=2)
    for fb, flags in zip(fbs, (flags_a, b["flags"])):
        want = R.truncated_world(vxo, w, flags).render(p, fb=np.zeros((H2, W2, 4), np.uint8), nthreads=16)["fb"]
        assert np.array_equal(fb.cpu().numpy(), want)
    ctx.stream_close()
