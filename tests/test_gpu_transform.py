"""Stamp orientations on the device (include/vxrt.h, vxrt_transform_stamp): the bits and the summary equal to
tests/ref_transform.py for all 48 orientations on the edge shapes (source padding set, guard words behind the destination and
the summary), on the hand-derived cases of tests/transform_cases.py, the group law, the clipboard path through read_region,
edit_stamps, place_pieces and voxelize_mesh at two brick edges, capture and replay, a side stream, determinism, the host form,
every refusal in the documented order, the limit case of tests/transform_limit_cases.py beyond 2^32 bytes, and the headless
example's turn and mirror lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_region
from tests import ref_transform as R
from tests import ref_voxelize as RV
from tests import transform_cases as TC
from tests import transform_limit_cases as TL
from tests.helpers import eng, gen_dense, upload
from tests.test_transform_host import ALL, EDGE_SHAPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SGUARD = 0x5A5A5A5A, 0x55555555
i3 = lambda v: (C.c_int32 * 3)(*v)


def _o(vx, o):
    return vx.Orientation(tuple(o[0]), o[1])


def _dev(torch, words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to("cuda")


def _summary(words):
    w = np.ascontiguousarray(words).view(np.uint32)
    box = [int(v) for v in w[2:8].view(np.int32)]
    return int(w[0]) | int(w[1]) << 32, tuple(box[:3]), tuple(box[3:])


@pytest.fixture(scope="module")
def ctx(eng):
    """a context without a world: the call needs none"""
    vx, torch = eng
    c = vx.Context(0)
    yield c
    c.close()


def _raw(ctx, torch, src, sd, o, with_summary=True, stream=None):
    """the C call into guarded buffers; returns (destination words, summary tuple or None), the guards asserted"""
    dd = R.dims(o, sd)
    nw = (dd[0] + 31) // 32 * dd[1] * dd[2]
    out = torch.full((nw + 64,), GUARD, dtype=torch.int32, device="cuda")
    summ = torch.full((8 + 16,), SGUARD, dtype=torch.int32, device="cuda")
    import voxelengine_amd as vx
    desc = _o(vx, o)._c()
    rc = ctx._L.vxrt_transform_stamp(ctx._h, src.data_ptr(), i3(sd), C.byref(desc), out.data_ptr(), summ.data_ptr() if with_summary else None,
                                     stream)
    assert rc == 0, ctx._L.vxrt_last_error()
    torch.cuda.synchronize()
    assert bool((out[nw:] == GUARD).all()) and bool((summ[8 if with_summary else 0:] == SGUARD).all())
    return out[:nw].cpu().numpy().view(np.uint32), _summary(summ[:8].cpu().numpy()) if with_summary else None


@pytest.mark.parametrize("sd", EDGE_SHAPES)
def test_bit_equal_for_all_48_orientations(eng, ctx, sd):
    """source padding bits set; bits, cleared padding and summary equal to the restatement; guard words untouched; without a
    summary the bits are the same"""
    vx, torch = eng
    g = np.random.default_rng(sum(sd)).random(sd) < 0.3
    src = _dev(torch, R.pack_padded(g))
    bad = []
    for i, o in enumerate(ALL):
        want = R.transform(g, o)
        words, got = _raw(ctx, torch, src, sd, o)
        bits, pad = R.unpack(words, want.shape)
        if not (np.array_equal(bits, want) and not pad.any() and got == R.summary(want)):
            bad.append((o, int((bits != want).sum()), int(pad.sum()), got, R.summary(want)))
        if i % 6 == 0:
            plain, none = _raw(ctx, torch, src, sd, o, with_summary=False)
            assert none is None and np.array_equal(plain, words), o
    print("transform", sd, "orientations wrong:", bad)
    assert not bad


def test_hand_derived_cases_and_the_host_form(eng, ctx):
    vx, torch = eng
    for case in TC.written_out():
        words, got = _raw(ctx, torch, _dev(torch, np.asarray(case["words"], np.uint32)), case["dims"], case["o"])
        TC.check(case, case["want_dims"], words)
        grid = R.unpack(words, case["want_dims"])[0]
        assert got == R.summary(grid)
        host = ctx.transform_stamp_host(TC.source_grid(case), _o(vx, case["o"]))
        assert host.dims == tuple(case["want_dims"]) and np.array_equal(host.bits, grid) and tuple(host.summary) == got
    # the host form takes padded words as they are, and works without a summary
    g = np.random.default_rng(4).random((33, 5, 65)) < 0.4
    src = R.pack_padded(g)
    for o in ALL[::7]:
        want = R.transform(g, o)
        dst, summ = np.full(len(R.pack(want)) + 4, GUARD, np.uint32), np.full(12, SGUARD, np.uint32)
        desc = _o(vx, o)._c()
        for s in (summ.ctypes.data, None):
            assert ctx._L.vxrt_transform_stamp_host(ctx._h, src.ctypes.data, i3(g.shape), C.byref(desc), dst.ctypes.data, s) == 0
            assert np.array_equal(dst[:-4], R.pack(want)) and (dst[-4:] == GUARD).all()
        assert _summary(summ[:8]) == R.summary(want) and (summ[8:] == SGUARD).all()


def test_the_group_law_on_the_device(eng, ctx):
    """by a and then by b is by a.then(b), for all 48 x 48 pairs; by o and then by o.inverse() is the source, padding cleared"""
    vx, torch = eng
    g = np.random.default_rng(11).random((33, 5, 34)) < 0.4
    src, clean = _dev(torch, R.pack_padded(g)), _dev(torch, R.pack(g))
    once = {o: ctx.transform_stamp(src, g.shape, _o(vx, o), summary=False) for o in ALL}
    wrong = []
    for a in ALL:
        for b in ALL:
            ab = _o(vx, a).then(_o(vx, b))
            twice = ctx.transform_stamp(once[a].bits, once[a].dims, _o(vx, b), summary=False)
            want = once[(tuple(ab.axis), ab.flip)]
            if twice.dims != want.dims or not torch.equal(twice.bits, want.bits):
                wrong.append((a, b))
        back = ctx.transform_stamp(once[a].bits, once[a].dims, _o(vx, a).inverse())
        assert back.dims == g.shape and torch.equal(back.bits, clean), a
        assert tuple(back.summary) == R.summary(g)
    assert not wrong, wrong[:10]


def test_the_summary_of_empty_full_and_single_voxel_stamps(eng, ctx):
    vx, torch = eng
    sd = (65, 33, 34)
    for o in ALL[::5]:
        r = ctx.transform_stamp(torch.zeros(vx.region_words(sd), dtype=torch.int32, device="cuda"), sd, _o(vx, o))
        assert tuple(r.summary) == (0, (R.INT32_MAX,) * 3, (R.INT32_MIN,) * 3) and not bool(r.bits.any())
        # only padding set: still empty
        pad = _dev(torch, R.pack_padded(np.zeros(sd, bool)))
        r = ctx.transform_stamp(pad, sd, _o(vx, o))
        assert tuple(r.summary) == (0, (R.INT32_MAX,) * 3, (R.INT32_MIN,) * 3) and not bool(r.bits.any())
        full = ctx.transform_stamp(_dev(torch, R.pack_padded(np.ones(sd, bool))), sd, _o(vx, o))
        dd = R.dims(o, sd)
        assert tuple(full.summary) == (65 * 33 * 34, (0, 0, 0), tuple(d - 1 for d in dd)) and full.grid().all()
        for p in [(64, 32, 33), (0, 0, 0), (32, 31, 5)]:
            one = np.zeros(sd, bool)
            one[p] = True
            r = ctx.transform_stamp(_dev(torch, R.pack_padded(one)), sd, _o(vx, o))
            q = _o(vx, o).voxel(p, sd)
            assert tuple(r.summary) == (1, q, q) and q == R.voxel(o, sd, p) and r.grid()[q]
        assert ctx.transform_stamp(pad, sd, _o(vx, o), summary=False).summary is None


@pytest.mark.parametrize("factor", [8, 16])
def test_the_clipboard_path(eng, vxo, factor):
    """read_region, transform_stamp, edit_stamps equals the same on a dense grid; a turned piece in place_pieces overlaps what the
    turned grid overlaps; a voxelized mesh turned on the device is the restatement's turn of its bits"""
    vx, torch = eng
    rng = np.random.default_rng(factor)
    edge = 8 * factor
    vox = rng.random((edge, edge, edge)) < 0.3
    c = vx.Context(0)
    try:
        upload(c, vxo.World.from_voxels(vox, factor))
        cur = vox
        for k, o in enumerate([ALL[i] for i in (1, 10, 19, 28, 37, 46, 8, 23)]):
            origin, d = (int(rng.integers(-5, edge - 20)), int(rng.integers(0, edge - 30)), int(rng.integers(-3, edge - 10))), (33 + k, 9 + 2 * k, 17)
            clip = c.read_region(origin, d)
            turned = c.transform_stamp(clip, d, _o(vx, o))
            want = R.transform(ref_region.read_region(cur, origin, d), o)
            assert turned.dims == want.shape and tuple(turned.summary) == R.summary(want)
            # the fit test before the paste: the turned piece against the world at the place it will go
            at = (int(rng.integers(-8, edge - 8)), int(rng.integers(-8, edge - 8)), int(rng.integers(-8, edge - 8)))
            placed = c.place_pieces([turned.piece()], [vx.Placement(0, at, 1, 0)]).cpu().numpy()
            assert int(placed[0, 0]) == int((ref_region.read_region(cur, at, want.shape) & want).sum())
            mode = k % 3
            c.edit_stamps([turned.stamp(at, mode)])
            cur = ref_region.apply_stamps(cur, [(at, want, mode)])
            assert np.array_equal(c.read_region_host((0, 0, 0), (edge, edge, edge)), cur), (k, o)
        # a voxelized mesh
        dims = (40, 33, 21)
        verts, tris = RV.octahedron((20 * 256 + 128, 16 * 256, 10 * 256 + 77), 9 * 256 + 30)
        mesh = c.voxelize_mesh(verts, tris, dims)
        bits = mesh.grid()
        assert bits.any()
        for o in ALL[2::9]:
            r = c.transform_stamp(mesh.bits, dims, _o(vx, o))
            assert np.array_equal(r.grid(), R.transform(bits, o)) and tuple(r.summary) == R.summary(R.transform(bits, o))
    finally:
        c.close()


def test_works_beside_a_streamed_world(eng, vxo, tmp_path):
    vx, torch = eng
    c = vx.Context(0)
    try:
        upload(c, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        path = str(tmp_path / "s.vxb")
        c.save_world(path)
        c.stream_open(path, 1000)
        g = np.random.default_rng(2).random((40, 7, 33)) < 0.5
        r = c.transform_stamp(_dev(torch, R.pack_padded(g)), g.shape, _o(vx, ALL[29]))
        assert np.array_equal(r.grid(), R.transform(g, ALL[29]))
        c.stream_close()
    finally:
        c.close()


def test_capture_replay_side_stream_and_determinism(eng, ctx):
    """both kernels captured into one graph on a side stream and replayed over poisoned outputs and a changed source; the same
    launches on the side stream directly; two calls bit-identical"""
    vx, torch = eng
    rng = np.random.default_rng(6)
    sd = (97, 33, 40)
    g = rng.random(sd) < 0.4
    src = _dev(torch, R.pack_padded(g))
    jobs = []
    for o in (ALL[3], ALL[20], ALL[41]):  # rows moved whole, and both transposed axes
        dd = R.dims(o, sd)
        jobs.append(dict(o=o, desc=_o(vx, o)._c(), dd=dd, bits=torch.zeros(vx.region_words(dd), dtype=torch.int32, device="cuda"),
                         summ=torch.zeros(8, dtype=torch.int32, device="cuda")))
    side = torch.cuda.Stream()
    L, h = ctx._L, ctx._h

    def issue():
        for j in jobs:
            assert L.vxrt_transform_stamp(h, src.data_ptr(), i3(sd), C.byref(j["desc"]), j["bits"].data_ptr(), j["summ"].data_ptr(),
                                          side.cuda_stream) == 0

    def check(grid, tag):
        for j in jobs:
            want = R.transform(grid, j["o"])
            assert np.array_equal(vx.unpack_region(j["bits"], j["dd"]), want), (tag, j["o"])
            assert _summary(j["summ"].cpu().numpy()) == R.summary(want), (tag, j["o"])

    def poison():
        for j in jobs:
            j["bits"].fill_(GUARD)
            j["summ"].fill_(GUARD)

    with torch.cuda.stream(side):
        poison()
        issue()
        side.synchronize()
    check(g, "side stream")
    first = [(j["bits"].clone(), j["summ"].clone()) for j in jobs]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        issue()
    for grid in (g, ~g):
        with torch.cuda.stream(side):
            src.copy_(_dev(torch, R.pack_padded(grid)))
            poison()
            graph.replay()
            side.synchronize()
        check(grid, "replay")
        if grid is g:
            for j, (b, s) in zip(jobs, first):
                assert torch.equal(j["bits"], b) and torch.equal(j["summ"], s)
    torch.cuda.synchronize()
    a = ctx.transform_stamp(src, sd, _o(vx, ALL[20]))
    b = ctx.transform_stamp(src, sd, _o(vx, ALL[20]), stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(a.bits, b.bits) and a.summary == b.summary


def test_refusals_in_the_documented_order_leave_the_outputs_untouched(eng):
    vx, torch = eng
    c = vx.Context(0)  # no world: none is needed, and no refusal names one
    try:
        L, h = c._L, c._h
        sd = (33, 4, 4)
        n = vx.region_words(sd)
        buf = torch.full((1024,), GUARD, dtype=torch.int32, device="cuda")
        summ = torch.full((8,), SGUARD, dtype=torch.int32, device="cuda")
        src, dst = buf.data_ptr(), buf.data_ptr() + 4 * 512
        hbuf, hsum = np.full(1024, GUARD, np.uint32), np.full(8, SGUARD, np.uint32)
        hsrc, hdst = hbuf.ctypes.data, hbuf.ctypes.data + 4 * 512
        good = vx.Orientation.rotation(2, 1)._c()
        bad_o = vx.Orientation((0, 0, 2), 9)._c()
        bad_flip = vx.Orientation((0, 1, 2), 8)._c()
        bad_d, over = i3((0, 4, 4)), i3(TL.OVER_CAP_DIMS)

        def dev(s=src, d=i3(sd), o=good, t=dst):
            return L.vxrt_transform_stamp(h, s, d, C.byref(o) if o is not None else None, t, summ.data_ptr(), None)

        def host(s=src, d=i3(sd), o=good, t=dst):  # (the same offsets into the host buffer)
            s = None if s is None else hsrc + (s - src)
            t = None if t is None else hsrc + (t - src)
            return L.vxrt_transform_stamp_host(h, s, d, C.byref(o) if o is not None else None, t, hsum.ctypes.data)

        def refused(why, **kw):
            for call in (dev, host):
                assert call(**kw) == -1, kw
                assert why in L.vxrt_last_error().decode(), (why, L.vxrt_last_error())

        def untouched():
            torch.cuda.synchronize()
            return bool((buf == GUARD).all()) and bool((summ == SGUARD).all()) and (hbuf == GUARD).all() and (hsum == SGUARD).all()

        assert L.vxrt_transform_stamp(None, src, i3(sd), C.byref(good), dst, None, None) == -1
        assert "ctx is NULL" in L.vxrt_last_error().decode()
        assert L.vxrt_transform_stamp_host(None, hsrc, i3(sd), C.byref(good), hdst, None) == -1
        # each check comes before every later one
        for k in ("s", "d", "o", "t"):
            refused("NULL argument", **{"o": bad_o, "d": bad_d, "t": src, k: None})
        refused("orientation", o=bad_o, d=bad_d, t=src)
        refused("orientation", o=bad_flip, d=over, t=src)
        for d in [(0, 4, 4), (4, -1, 4), (1 << 20, 1 << 16, 2)]:
            refused("src_dims", d=i3(d), t=src)
        refused("VXRT_TRANSFORM_MAX_WORDS", d=over, t=src)
        refused("VXRT_TRANSFORM_MAX_WORDS", d=i3((32, 1, 2 ** 31 - 1)), t=src)  # the destination alone: 32 rows of one voxel each
        refused("overlap", t=src)
        refused("overlap", t=src + 4 * (n - 1))
        refused("overlap", s=src + 4 * 131, t=src)  # the turned stamp is 4 x 33 x 4: 132 words
        assert untouched()
        with pytest.raises(vx.VxrtError, match="overlap"):
            c.transform_stamp(buf, sd, vx.Orientation.rotation(2, 1), out=buf)
        with pytest.raises(ValueError):
            c.transform_stamp(buf[:n - 1], sd, vx.Orientation())
        assert dev(s=src + 4 * 132, t=src) == 0 and host(s=src + 4 * 132, t=src) == 0 and dev() == 0 and host() == 0
        torch.cuda.synchronize()
        assert not untouched()
    finally:
        c.close()


def test_the_limit_case_beyond_2_32_bytes(eng, ctx):
    """tests/transform_limit_cases.py: a source of more than 2^32 bytes in about 2^30 voxels, a pattern made on the device; the
    round trip through the inverse returns it with its padding cleared, and sampled voxels and the eight corners obey the index
    rule"""
    vx, torch = eng
    sd = TL.LIMIT_DIMS
    n = vx.region_words(sd)
    assert 4 * n > 1 << 32
    free, _ = torch.cuda.mem_get_info()
    need = 4 * n * 6  # the source, its clean copy, the pattern's temporaries, a destination and the round trip
    if free < need:
        pytest.skip("the card has %d bytes free, the case needs %d" % (free, need))
    src = TL.pattern_words(torch, n)
    clean = src & 1
    total = int(clean.sum(dtype=torch.int64))
    assert n // 4 < total < 3 * n // 4
    rng = np.random.default_rng(0)
    pts = [(0, y, z) for y in (0, sd[1] - 1) for z in (0, sd[2] - 1)] * 2
    pts += [(0, int(rng.integers(0, sd[1])), int(rng.integers(0, sd[2]))) for _ in range(4000)]
    pts += [(0, sd[1] - 1, sd[2] - 1), (0, 4095, sd[2] - 1)]  # word indices at and beyond 2^30
    want = np.asarray([TL.pattern_bit(p[1] + sd[1] * p[2]) for p in pts], np.int64)
    assert 1000 < want.sum() < 3000
    for o in TL.LIMIT_ORIENTATIONS:
        r = ctx.transform_stamp(src, sd, _o(vx, o))
        dd = r.dims
        assert dd == R.dims(o, sd) and tuple(r.summary)[0] == total
        qs = np.asarray([R.voxel(o, sd, p) for p in pts], np.int64)
        word = (qs[:, 1] + dd[1] * qs[:, 2]) * ((dd[0] + 31) // 32) + (qs[:, 0] >> 5)
        got = (r.bits[torch.from_numpy(word).to("cuda")].cpu().numpy().view(np.uint32) >> (qs[:, 0] & 31).astype(np.uint32)) & 1
        assert np.array_equal(got.astype(np.int64), want), o
        back = ctx.transform_stamp(r.bits, dd, _o(vx, o).inverse(), summary=False)
        assert back.dims == sd and torch.equal(back.bits, clean), o
        del r, back


def test_headless_example_turn_and_mirror_lines(vxo, tmp_path):
    """examples/voxelapp_headless: copy, turn, mirror, paste; the printed dims, voxels, bounds and hash are those of the restated
    stamp and the frame rendered afterwards is the oracle's frame of the restated world"""
    from oracle import vxo_edit
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge, W_, H_ = 256, 64, 48
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    heights = np.where(vox.any(1), edge - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
    top = int(np.median(heights[100:160, 100:150]))
    a, d, at = (100, top - 20, 100), (60, 45, 37), (70, top + 3, 60)
    sf = tmp_path / "edits.txt"
    sf.write_text("0 2 0 %d %d %d %d %d %d\n0 turn 2 1\n0 mirror 1 0\n0 turn 0 -1 0\n0 3 0 %d %d %d 0 0 0\n" % (*a, *d, *at))
    pos, euler = (64.0, float(top + 40), 64.0), (-0.45, 0.7, 0.0)
    path = tmp_path / "path.txt"
    path.write_text("%r %r %r %r %r %r\n" % (*pos, *euler))
    prefix = str(tmp_path / "tm")
    out = subprocess.run([exe, str(edge), "0", prefix, str(W_), str(H_), "2", str(path), "1", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    clip, want = ref_region.read_region(vox, a, d), []
    for what, o in (("turn", R.rotation(2, 1)), ("mirror", ((0, 1, 2), 2)), ("turn", R.rotation(0, -1))):
        clip = R.transform(clip, o)
        n, lo, hi = R.summary(clip)
        h = 0xcbf29ce484222325
        for b in R.pack(clip).tobytes():
            h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        want.append("%s before frame 0: slot 0, dims %d %d %d, %d voxels, box %d %d %d %d %d %d, hash %016x" % (what, *clip.shape, n, *lo, *hi, h))
    assert clip.any() and clip.shape != d
    lines = [x for x in out.stdout.splitlines() if x.startswith(("turn before", "mirror before"))]
    assert lines == want, out.stdout
    assert out.stdout.count("copy before frame") == 1 and out.stdout.count("paste before frame") == 1
    w = vxo.World.from_dense(vxo.dense_from_voxels(ref_region.apply_stamps(vox, [(at, clip, 0)])), edge, edge, edge, 32)
    f, u, r = vxo.get_directions(euler)
    p = vxo.make_params(W_, H_, tuple(np.float32(v) for v in pos), f, u, r, frame_number=0, mode=vxo.MODE_SHADED, checkerboard=0,
                        shadow=1, bounce_samples=1)
    fb = w.render(p, fb=np.full((H_, W_, 4), 255, np.uint8), nthreads=16)["fb"]
    raw = open("%s_0000.ppm" % prefix, "rb").read()
    head = b"P6\n%d %d\n255\n" % (W_, H_)
    assert raw.startswith(head)
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(H_, W_, 3), fb[:, :, [2, 1, 0]])
    plain = vxo.World.from_dense(vxo.dense_from_voxels(vox), edge, edge, edge, 32).render(p, fb=np.full((H_, W_, 4), 255, np.uint8), nthreads=16)["fb"]
    assert not np.array_equal(plain, fb)  # the pasted stamp is in view
