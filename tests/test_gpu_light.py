"""Voxel light fields on the device (include/vxrt.h, vxrt_light_field): the levels and the summary equal to
tests/ref_light.py on leaky-roof worlds at every brick edge, box width, channel mask and emitter class, on the hand-derived
cases of tests/light_cases.py, on every world path, after edits and stamps, on a bench-world window whose columns run to the
world's top and at the ends of int32; determinism across calls and streams; the host form; guard bytes; every refusal in
the documented order, leaving the outputs untouched; and the headless example's light lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_edit, ref_region
from tests import light_cases as LC
from tests import ref_light as R
from tests.helpers import eng, gen_dense, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
MASKS = (R.SKY, R.BLOCK, R.SKY | R.BLOCK)
WIDTHS = (1, 4, 5, 36, 37, 100)


def _assert_field(ctx, world, origin, dims, emitters=None, channels=R.SKY | R.BLOCK, stream=None, shift=(0, 0, 0)):
    """the device field against the reference computed on `world`, whose (0, 0, 0) is world voxel `shift`"""
    r = ctx.light_field(origin, dims, emitters, channels, stream=stream)
    moved = None if emitters is None else [(x - shift[0], y - shift[1], z - shift[2], l) for x, y, z, l in emitters]
    want = R.light_field(world, tuple(np.asarray(origin) - np.asarray(shift)), dims, moved, channels)
    got = r.grid()
    print("light", origin, dims, channels, tuple(r.summary), int((got != want["levels"]).sum()))
    assert np.array_equal(got, want["levels"]), (origin, dims, channels)
    assert tuple(r.summary) == want["summary"], (origin, dims, channels)
    return r, want


def _emitters(rng, world, o, d, n=24):
    """entries of all four classes around the box, with duplicates: random ones (levels 0 .. 16), one certainly invalid, one
    certainly far, one of level 15 in an empty voxel of the box"""
    lo, hi = [v - 20 for v in o], [v + s + 20 for v, s in zip(o, d)]
    e = [(*(int(rng.integers(lo[k], hi[k])) for k in range(3)), int(rng.integers(0, 17))) for _ in range(n)]
    a = [max(v, 0) for v in o]
    b = [min(v + s, w) for v, s, w in zip(o, d, world.shape)]
    free = np.argwhere(~world[a[0]:b[0], a[1]:b[1], a[2]:b[2]])
    sure = (*(int(v) + l for v, l in zip(free[len(free) // 2], a)), 15)
    return e + e[:3] + [(lo[0], lo[1], lo[2], 16), (hi[0] + 100, hi[1], hi[2], 7), sure]


@pytest.mark.parametrize("factor,edge", [(8, 64), (16, 128), (32, 256)])
def test_field_equals_the_reference(eng, vxo, factor, edge):
    vx, torch = eng
    rng = np.random.default_rng(factor)
    roof = edge // 2
    vox = R.leaky_roof_world(rng, shape=(edge, edge, edge), roof_y=roof)
    boxes = [((3, roof - 9, 5), (1, 20, 9)), ((-7, roof - 4, -3), (4, 12, 11)), ((edge - 3, roof - 12, 9), (5, 17, 6)),
             ((11, roof - 10, edge - 20), (36, 15, 30)), ((-20, roof - 6, 17), (37, 13, 5)), ((edge - 70, roof - 8, 1), (100, 11, 7)),
             ((-5, roof - 20, -3), (edge + 10, 30, 70))]
    assert tuple(d[0] for _, d in boxes[:6]) == WIDTHS
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, factor))
        levels_seen, classes = [set(), set()], np.zeros(4, np.int64)
        for o, d in boxes:
            e = _emitters(rng, vox, o, d)
            for channels in MASKS:
                r, want = _assert_field(ctx, vox, o, d, e, channels)
                if channels == R.SKY | R.BLOCK:
                    s = want["summary"]
                    classes += s[6:10]
                    for c in range(2):
                        levels_seen[c] |= {l for l in range(16) if s[2 + c][l]}
        assert levels_seen[0] == set(range(16)) and levels_seen[1] == set(range(16))
        assert classes.min() > 0  # every class of emitter
    finally:
        ctx.close()


def test_hand_derived_cases(eng, vxo):
    vx, torch = eng
    for case in LC.all_cases():
        ctx = vx.Context(0)
        try:
            upload(ctx, vxo.World.from_voxels(case["world"], 8))
            for channels in MASKS:
                r = ctx.light_field(case["origin"], case["dims"], case["emitters"], channels)
                LC.check(case, {"levels": r.grid(), "summary": tuple(r.summary)}, channels)
        finally:
            ctx.close()


def test_every_world_path(eng, vxo, tmp_path):
    """a world built on the device, the same world saved and loaded into a second context, and its tables uploaded into a
    third: one field, equal to the reference on the world read back"""
    vx, torch = eng
    a, b, c = vx.Context(0), vx.Context(0), vx.Context(0)
    try:
        a.build_world(vx.GEN_INT_TERRAIN, 256, 256, 256, 32)
        vox = a.read_region_host((0, 0, 0), (256, 256, 256))
        heights = np.where(vox.any(1), 255 - np.argmax(vox[:, ::-1, :], axis=1), 0)
        o, d = (-6, max(int(np.median(heights)) - 20, 0), 150), (100, 40, 120)
        e = _emitters(np.random.default_rng(2), vox, o, d)
        first, want = _assert_field(a, vox, o, d, e)
        assert want["summary"][0] > 1000 and sum(want["summary"][2][1:]) > 1000
        path = str(tmp_path / "w.vxb")
        a.save_world(path)
        b.load_world(path)
        w = a.download_world()
        c.upload_world(w["factor"], w["cdims"], w["coarse_bits"], w["brick_slot"], w["bounds"], w["pool"])
        for other in (b, c):
            r = other.light_field(o, d, e)
            assert np.array_equal(r.grid(), first.grid()) and r.summary == first.summary
    finally:
        for ctx in (a, b, c):
            ctx.close()


def test_field_follows_edits_and_stamps(eng, vxo):
    """a cave under a roof: dark; edit_voxels opens a hole in the roof and light falls in; edit_stamps closes it again"""
    vx, torch = eng
    vox = np.zeros((128, 128, 128), bool)
    vox[:, :20, :] = True
    vox[:, 40:44, :] = True
    rng = np.random.default_rng(4)
    vox[:, 20:40, :] = rng.random((128, 20, 128)) < 0.2
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (30, 18, 35), (60, 22, 50)  # up to the roof's underside
        lamp = [(60, 30, 60, 12)] if not vox[60, 30, 60] else [(60, 31, 60, 12)]
        before, want = _assert_field(ctx, vox, o, d, lamp)
        assert want["summary"][1] == 0 and sum(want["summary"][2][1:]) == 0  # sealed under the roof: no sky light
        ops = [(0, 0, (58, 40, 58), (61, 43, 61))]
        # no synchronisation between the edit and the field: the call orders after the work queued on the stream
        ctx.edit_voxels([vx.EditBox(a, b, v) for k, v, a, b in ops])
        opened = ref_edit.apply_edits(vox, ops)
        r, want = _assert_field(ctx, opened, o, d, lamp)
        assert want["summary"][1] > 0 and all(want["summary"][2][l] > 0 for l in range(1, 16))
        stamps = [((56, 41, 56), np.ones((8, 2, 8), bool), vx.STAMP_UNION)]
        ctx.edit_stamps([vx.Stamp(so, m, mode) for so, m, mode in stamps])
        closed = ref_region.apply_stamps(opened, stamps)
        r, want = _assert_field(ctx, closed, o, d, lamp)
        assert want["summary"][1] == 0 and np.array_equal(r.sky(), before.sky()) and (r.sky() == 0).all()
    finally:
        ctx.close()


def test_bench_world_window(eng):
    """a 64 x 96 x 64 window of the bench world at the terrain surface; the reference works on read_region_host of the halo
    and of its columns up to the world's top"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, 8192, 512, 8192, 32)
        ox, oz = 4000, 3000
        col = ctx.read_region_host((ox, 0, oz), (64, 512, 64))
        heights = np.where(col.any(1), 511 - np.argmax(col[:, ::-1, :], axis=1), 0)
        o, d = (ox, max(int(np.median(heights)) - 48, 14), oz), (64, 96, 64)
        shift = tuple(v - 14 for v in o)
        world = ctx.read_region_host(shift, (d[0] + 28, 512 - shift[1], d[2] + 28))  # voxel 0 at shift, up to the world's top
        assert shift[1] + world.shape[1] == 512 and world.shape[1] > d[1] + 28
        rng = np.random.default_rng(6)
        e = [(o[0] + int(rng.integers(0, 64)), o[1] + int(rng.integers(0, 96)), o[2] + int(rng.integers(0, 64)), int(rng.integers(1, 16)))
             for _ in range(64)]
        for channels in MASKS:
            r, want = _assert_field(ctx, world, o, d, e, channels, shift=shift)
        s = want["summary"]
        assert s[0] > 10000 and s[1] > 10000 and s[6] > 0
    finally:
        ctx.close()


def test_boxes_at_the_ends_of_int32(eng, vxo):
    """the last origins whose halo fits in int32, far from the world: every voxel exposed, sky 15; one voxel further is
    refused"""
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        d = (37, 9, 5)
        n = d[0] * d[1] * d[2]
        hist = lambda l: tuple(n if k == l else 0 for k in range(16))
        for k in range(3):
            for edge, step in [(INT32_MIN + 14, -1), (INT32_MAX - d[k] - 14, 1)]:
                o = [300, 300, 300]  # beside the world in x and z: exposed at any height
                o[k] = edge
                lamp = [(o[0], o[1], o[2], 3), (5, 5, 5, 9)]
                f = ctx.light_field(o, d, lamp)
                want = np.full(d, 15 << 4, np.uint8)
                want[0, 0, 0], want[1, 0, 0], want[0, 1, 0], want[0, 0, 1], want[2, 0, 0], want[0, 2, 0] = 0xF3, 0xF2, 0xF2, 0xF2, 0xF1, 0xF1
                want[1, 1, 0] = want[1, 0, 1] = want[0, 1, 1] = want[0, 0, 2] = 0xF1
                assert np.array_equal(f.grid(), want)
                s = f.summary
                assert (s.solid, s.exposed, s.hist_sky, s.sum_sky, s.sum_block) == (0, n, hist(15), 15 * n, 3 + 3 * 2 + 6)
                assert (s.emitters_used, s.emitters_solid, s.emitters_far, s.emitters_invalid) == (1, 0, 1, 0)
                o[k] = edge + step
                with pytest.raises(vx.VxrtError):
                    ctx.light_field(o, d)
    finally:
        ctx.close()


def test_deterministic_across_calls_and_streams_and_host_form(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(5)
    vox = R.leaky_roof_world(rng, shape=(128, 128, 128), roof_y=70)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 16))
        o, d = (-5, 50, 7), (120, 40, 110)
        e = _emitters(rng, vox, o, d, n=200)
        for channels in MASKS:
            first = ctx.light_field(o, d, e, channels)
            side = torch.cuda.Stream()
            for k in range(3):
                s = side.cuda_stream if k == 2 else None
                r = ctx.light_field(o, d, e, channels, stream=s)
                if s is not None:
                    side.synchronize()
                assert r.summary == first.summary and torch.equal(r.levels, first.levels)
            host = ctx.light_field_host(o, d, e, channels)
            assert np.array_equal(host.grid(), first.grid()) and host.summary == first.summary
            want = R.light_field(vox, o, d, e, channels)
            assert tuple(first.summary) == want["summary"] and np.array_equal(first.grid(), want["levels"])
    finally:
        ctx.close()


def test_guard_bytes_behind_the_output_and_the_workspace(eng, vxo):
    vx, torch = eng
    rng = np.random.default_rng(7)
    vox = R.leaky_roof_world(rng, shape=(64, 64, 64), roof_y=30)
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        for o, d in [((-3, 20, 5), (37, 21, 13)), ((40, 25, -9), (5, 7, 3)), ((0, 0, 0), (64, 64, 64))]:
            n = d[0] * d[1] * d[2]
            e = _emitters(rng, vox, o, d)
            for channels in MASKS:
                ws = ctx.light_workspace_bytes(d, channels)
                work = torch.full((ws + 256,), 0xA5, dtype=torch.uint8, device="cuda")
                out = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
                r = ctx.light_field(o, d, e, channels, out=out, work=work)
                want = R.light_field(vox, o, d, e, channels)
                assert np.array_equal(r.grid(), want["levels"]) and tuple(r.summary) == want["summary"]
                assert bool((out[n:] == 0x5A).all()) and bool((work[ws:] == 0xA5).all())
    finally:
        ctx.close()


def test_refusals_in_the_documented_order_leave_the_outputs_untouched(eng, vxo, tmp_path):
    vx, torch = eng
    ctx = vx.Context(0)
    try:
        L, h = ctx._L, ctx._h
        ws = ctx.light_workspace_bytes((8, 8, 8), 3)
        assert ws > 0
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        out = torch.full((512,), 0x5A, dtype=torch.uint8, device="cuda")
        summ = torch.full((42,), 0x55, dtype=torch.int32, device="cuda")
        em = torch.tensor([[3, 3, 3, 9]], dtype=torch.int32, device="cuda")
        hem = np.array([[3, 3, 3, 9]], np.int32)
        i3 = lambda *v: (C.c_int32 * 3)(*v)
        o3, d3 = i3(0, 0, 0), i3(8, 8, 8)
        hout, hsum = np.full(512, 0x5A, np.uint8), np.full(42, 0x55, np.uint32)

        def field(o=o3, d=d3, e=em.data_ptr(), n=1, c=3, wk=work.data_ptr(), ot=out.data_ptr(), s=summ.data_ptr()):
            return L.vxrt_light_field(h, o, d, e, n, c, wk, ot, s, None)

        def host(o=o3, d=d3, e=hem.ctypes.data, n=1, c=3, ot=hout.ctypes.data, s=hsum.ctypes.data):
            return L.vxrt_light_field_host(h, o, d, e, n, c, ot, s)

        def untouched():
            torch.cuda.synchronize()
            return bool((out == 0x5A).all()) and bool((summ == 0x55).all()) and (hout == 0x5A).all() and (hsum == 0x55).all()

        def refused(why, **kw):
            """both forms refuse with VXRT_ERR_INVALID and the message of the check `why`"""
            for call in (field, host):
                assert call(**kw) == -1, kw
                assert why in L.vxrt_last_error().decode(), (why, L.vxrt_last_error())

        bad_d, bad_o, far_o = i3(0, 8, 8), i3(INT32_MAX - 21, 0, 0), i3(INT32_MAX - 22, 0, 0)
        assert field() == -3 and host() == -3 and untouched()    # no world
        # each check comes before every later one, and before the missing world
        for k in ("o", "d", "wk", "ot", "s"):
            assert field(**{"c": 0, "n": 70000, "d": bad_d, k: None}) == -1, k
            assert "NULL argument" in L.vxrt_last_error().decode()
        for k in ("o", "d", "ot", "s"):
            assert host(**{"c": 0, "n": 70000, "d": bad_d, k: None}) == -1, k
            assert "NULL argument" in L.vxrt_last_error().decode()
        assert L.vxrt_light_field(None, o3, d3, em.data_ptr(), 1, 3, work.data_ptr(), out.data_ptr(), summ.data_ptr(), None) == -1
        for c in (0, 4, 7, 2 ** 32 - 1):
            refused("channels", c=c, n=70000, d=bad_d, o=bad_o)
        refused("VXRT_LIGHT_MAX_EMITTERS", n=65537, d=bad_d, o=bad_o)
        refused("VXRT_LIGHT_MAX_EMITTERS", n=65537, c=1)                     # checked without the block channel too
        refused("emitters NULL", e=None, n=1, d=bad_d, o=bad_o)
        refused("emitters NULL", e=None, n=1, c=2)
        for bad in [(0, 8, 8), (8, -1, 8), (1024, 1024, 257), (1, 1, 1 << 28)]:
            refused("box dims", d=i3(*bad), o=bad_o)
        refused("beyond int32", o=bad_o)
        refused("beyond int32", o=i3(0, INT32_MIN + 13, 0))
        assert field(o=far_o) == -3 and host(e=None, n=5, c=1) == -3         # valid arguments: the missing world is next
        assert untouched()
        upload(ctx, vxo.World.generate(vxo.GEN_INT_TERRAIN, 128, 128, 128, 16))
        refused("beyond int32", o=bad_o)
        path = str(tmp_path / "s.vxb")
        ctx.save_world(path)
        ctx.stream_open(path, 1000)
        refused("streamed")
        ctx.stream_close()
        assert untouched()
        ctx.load_world(path)
        assert field(e=None, n=5, c=1) == 0                                  # without the block channel the emitters are not read
        torch.cuda.synchronize()
        assert int(summ[38:].sum()) == 0 and not untouched()
        assert field() == 0 and host() == 0 and field(o=far_o) == 0 and field(n=0, e=None) == 0 and field(n=65536, e=None, c=1) == 0
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_headless_example_light_lines(vxo, tmp_path):
    """examples/voxelapp_headless kind 10: the printed summaries and the hash of the levels equal the reference's, for the sky
    channel at the surface and for both channels around the camera's cell, where the one emitter sits"""
    from oracle import vxo_edit
    exe = os.path.join(ROOT, "examples", "voxelapp_headless")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    edge = 256
    vox = vxo_edit.voxels_from_dense(gen_dense(vxo, vxo.GEN_PERLIN_REF, edge, edge, edge), edge, edge, edge)
    heights = np.where(vox.any(1), edge - 1 - np.argmax(vox[:, ::-1, :], axis=1), 0)
    top = int(np.median(heights[40:168, 0:95]))
    cam = (64, 230, 64)  # the cell of the example's camera: (edge / 4, 0.9 edge, edge / 4)
    jobs = [((40, max(top - 30, 0), -5), (100, 60, 70), 1), ((cam[0] - 20, cam[1] - 12, cam[2] - 20), (40, 30, 40), 3)]
    sf = tmp_path / "edits.txt"
    sf.write_text("".join("0 10 %d %d %d %d %d %d %d\n" % (c, *o, *d) for o, d, c in jobs))
    out = subprocess.run([exe, str(edge), "1", str(tmp_path / "lv"), "64", "48", "1", "-", "0", "1", "1", "0x0x0", str(sf)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr

    def fnv(data):
        h = 0xcbf29ce484222325
        for b in data:
            h = ((h ^ b) * 0x100000001b3) & (2 ** 64 - 1)
        return h
    want = []
    for o, d, c in jobs:
        r = R.light_field(vox, o, d, [(*cam, 15)] if c & 2 else None, c)
        s = r["summary"]
        want.append("light frame 0 solid %d exposed %d sky_sum %d block_sum %d used %d" % (s[0], s[1], s[4], s[5], s[6]))
        want.append("light hash frame 0 levels %016x" % fnv(r["levels"].transpose(2, 1, 0).tobytes()))
    assert not vox[cam] and "used 1" in want[2] and "used 0" in want[0]
    line = [x for x in out.stdout.splitlines() if x.startswith("light ")]
    assert line == want, out.stdout
