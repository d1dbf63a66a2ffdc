"""Light fields and piece queries on the device at the limits of their launches: the cases of tests/field_limit_cases.py,
each against tests/ref_light.py / tests/ref_place.py or a closed form that tests/test_field_limits_host.py holds against
them, and each with an assertion from the expected data that the call reached its path: emitters of every class in
workgroups past the first, every level in words past the first pass of the tally, an output off the dword grid, solid
voxels hundreds of slabs above the halo, a box of 2^28 voxels with an emitter on its last voxel, placements of a 2^20-lane
piece on both sides of the second grid row, blocked placements beside every cut of a batch, and placements past 65536
workgroups of one lane each."""
import ctypes as C

import numpy as np
import pytest

from tests import field_limit_cases as F
from tests import ref_light as RL
from tests import ref_place as RP
from tests.helpers import eng, upload
from tests.test_light_host import _expect_bytes
from tests.test_place_host import classes

pytestmark = pytest.mark.gpu


def _ctx(vx, vxo, vox, factor):
    ctx = vx.Context(0)
    upload(ctx, vxo.World.from_voxels(np.asarray(vox), factor))
    return ctx


def _assert_light(r, want, what):
    got = r.grid()
    print("light", what, tuple(r.summary), int((got != want["levels"]).sum()))
    assert np.array_equal(got, want["levels"]), what
    assert tuple(r.summary) == want["summary"], what


# ---- light
def test_emitters_over_256_workgroups(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    lanes = caps["classify_lanes"]
    e, cls, shared, special = F.emitter_list()
    o, d = F.EM_ORIGIN, F.EM_DIMS
    ctx = _ctx(vx, vxo, F.emitter_world(), 8)
    try:
        for n in F.EM_COUNTS:
            want = F.emitter_reference(n)
            # reached: entries past the first workgroup, used ones among them, that the field and the counts depend on
            assert n > lanes or n == min(F.EM_COUNTS)
            if n > lanes:
                assert cls[lanes:n].min() == 0 and want["summary"][6:10] != F.emitter_reference(lanes)["summary"][6:10]
                assert not np.array_equal(want["levels"], F.emitter_reference(lanes)["levels"])
            if n == max(F.EM_COUNTS):
                assert set(cls[lanes:].tolist()) == {0, 1, 2, 3} and (want["levels"][shared[0] - o[0], shared[1] - o[1], shared[2] - o[2]] & 15) == 15
            # a zeroed workspace: an emitter record that a launch failed to write then reads as "not used" instead of as a
            # plane word anywhere (dirty workspaces: tests/test_gpu_light.py, with lists of one workgroup)
            work = torch.zeros(ctx.light_workspace_bytes(d, 3), dtype=torch.uint8, device="cuda")
            for channels in (RL.SKY | RL.BLOCK, RL.BLOCK):
                r = ctx.light_field(o, d, torch.from_numpy(np.array(e[:n])).cuda(), channels, work=work)
                _assert_light(r, F.single_channel(want, channels), (n, channels))
    finally:
        ctx.close()


def test_tally_takes_a_second_pass(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    o, d = F.STRIDE_ORIGIN, F.STRIDE_DIMS
    want = F.stride_reference()
    past = F.tally_word_index(d, caps) >= F.tally_groups(d, caps)[1] * 256
    sky, block = F.levels_at(want["levels"], F.box_solid(F.stride_world(), o, d), past)
    assert sky == set(range(16)) and block == set(range(16))  # reached: every counter gets voxels in the second pass
    ctx = _ctx(vx, vxo, F.stride_world(), 16)
    try:
        for channels in F.MASKS:
            _assert_light(ctx.light_field(o, d, F.stride_emitters(), channels), F.single_channel(want, channels), channels)
    finally:
        ctx.close()


def test_tally_at_its_cap_of_workgroups(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    o, d = F.CAP_ORIGIN, F.CAP_DIMS
    sky, solid, exposed = F.cube_sky(o, d)
    past = F.tally_word_index(d, caps) >= caps["tally_max"] * 256
    assert set(sky[past & ~solid].tolist()) == set(range(16)) and solid[past].sum() == 64 * 64  # reached: passes 2 .. 9 count them
    want = RL.pack(sky, np.zeros_like(sky), solid, exposed, (0, 0, 0, 0))
    ctx = _ctx(vx, vxo, F.cube_world(), 8)
    try:
        for channels in (RL.SKY | RL.BLOCK, RL.SKY):
            _assert_light(ctx.light_field(o, d, None, channels), F.single_channel(want, channels), channels)
    finally:
        ctx.close()


def test_a_box_of_the_most_voxels(eng, vxo):
    """2^28 voxels around the cube, both channels, emitters in open air (one on the box's first voxel, one on its last):
    the output against the closed form slab by slab, the summary exactly, and guard bytes behind output and workspace"""
    vx, torch = eng
    o, d = F.MAXV_ORIGIN, F.MAXV_DIMS
    n = d[0] * d[1] * d[2]
    assert n == F.read_caps()["light_max_voxels"]
    lamps, counts = F.open_air_lamps(o, d, 32, 8)
    ctx = _ctx(vx, vxo, F.cube_world(), 8)
    try:
        ws = ctx.light_workspace_bytes(d, 3)
        assert ws == _expect_bytes(d, 3) and 1 << 28 < ws < 1 << 30
        assert ctx.light_workspace_bytes((d[0], d[1], d[2] + 1), 3) == 0
        work = torch.full((ws + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.full((n + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        r = ctx.light_field(o, d, lamps, 3, out=out, work=work)
        got = tuple(r.summary)
        total, plane, bad = F.SlabSummary(o, d, counts), d[0] * d[1], 0
        for z0 in range(0, d[2], F.MAXV_SLAB):
            z1 = z0 + F.MAXV_SLAB
            slab = F.cube_lamps_slab(o, d, lamps, z0, z1)
            total.add(slab, z0, z1)
            bad += int((out[z0 * plane:z1 * plane] != torch.from_numpy(slab.reshape(-1)).cuda()).sum())
        print("most voxels", got, bad)
        assert bad == 0
        assert got == total.summary() and got[0] == 64 ** 3 and got[6:10] == (32, 1, 1, 1)
        assert int(out[0]) == 0xFF and int(out[n - 1]) == 0xFE  # reached: the emitters on the first and the last voxel
        assert bool((out[n:] == 0x5A).all()) and bool((work[ws:] == 0xA5).all())
    finally:
        ctx.close()


def test_slabs_far_above_the_halo_and_the_clamp_below_the_world(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    o, d = F.ABOVE_ORIGIN, F.ABOVE_DIMS
    world = F.tall_world(caps)
    ctx = _ctx(vx, vxo, world, 8)
    try:
        want = RL.light_field(world, o, d, None, RL.SKY)
        r = ctx.light_field(o, d, None, RL.SKY)
        _assert_light(r, want, "tall")
        sky = r.sky()
        for (x, z), y in zip(F.ABOVE_COLUMNS, F.above_heights(caps)):  # reached: each voxel darkens its column, whatever its slab
            assert (sky[x - o[0], :, z - o[2]] == 14).all() and (sky[x - o[0] + 1, :, z - o[2]] == 15).all(), (x, y, z)
        assert int((sky == 14).sum()) == 4 * d[1] and int((sky == 15).sum()) == sky.size - 4 * d[1]
    finally:
        ctx.close()
    ctx = _ctx(vx, vxo, F.cube_world(), 8)
    try:
        for co, cd in F.CLAMP_BOXES:
            assert F.above_first(co, cd, caps) == 0 and F.above_slabs(F.CUBE, co, cd, caps) == F.CUBE // caps["light_slab"]
            want = RL.light_field(F.cube_world(), co, cd)
            assert np.array_equal(want["levels"], F.cube_field(co, cd)["levels"]) and want["summary"] == F.cube_field(co, cd)["summary"]
            _assert_light(ctx.light_field(co, cd), want, co)
        assert want["summary"][2][15] == 3 * 4 * 3 and want["summary"][2][14] == want["summary"][2][13] == 4 * 3  # x = -3 .. 1
    finally:
        ctx.close()


def test_output_off_the_dword_grid(eng, vxo):
    """d_levels at byte offsets 1, 2 and 3 of an allocation, through Context.light_field and through vxrt_light_field
    itself: the levels of the aligned call, 0x5A guard bytes before and behind untouched"""
    vx, torch = eng
    world = F.unaligned_world()
    ctx = _ctx(vx, vxo, world, 8)
    try:
        L, h = ctx._L, ctx._h
        i3 = lambda v: (C.c_int32 * 3)(*v)
        for o, d in F.UNALIGNED_BOXES:
            n = d[0] * d[1] * d[2]
            e = F.unaligned_emitters(o, d)
            want = RL.light_field(world, o, d, e)
            aligned = ctx.light_field(o, d, e)
            _assert_light(aligned, want, (o, d))
            assert want["summary"][6] == 3 and len(set(want["levels"].ravel().tolist())) > 3
            em = torch.tensor(e, dtype=torch.int32, device="cuda")
            work = torch.empty(ctx.light_workspace_bytes(d, 3), dtype=torch.uint8, device="cuda")
            for off in F.UNALIGNED_OFFSETS:
                big = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
                assert big.data_ptr() % 4 == 0
                out = big[off:off + n]
                assert out.data_ptr() % 4 == off  # reached: light_args clears `wide`
                r = ctx.light_field(o, d, e, out=out)
                _assert_light(r, want, (o, d, off))
                assert torch.equal(out, aligned.levels)
                assert bool((big[:off] == 0x5A).all()) and bool((big[off + n:] == 0x5A).all())
                raw = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
                summ = torch.zeros(42, dtype=torch.int32, device="cuda")
                assert (raw.data_ptr() + off) % 4 == off
                assert L.vxrt_light_field(h, i3(o), i3(d), em.data_ptr(), len(e), 3, work.data_ptr(), raw.data_ptr() + off,
                                          summ.data_ptr(), None) == 0
                torch.cuda.synchronize()
                assert torch.equal(raw, big) and RL.summary_from_words(summ.cpu().numpy()) == want["summary"]
    finally:
        ctx.close()


# ---- pieces
def _place(vx, torch, ctx, pieces, pl):
    out = ctx.place_pieces(pieces, torch.from_numpy(np.ascontiguousarray(pl, np.int32).reshape(-1, 6)).cuda())
    torch.cuda.synchronize()
    return out


def _mismatch(got, want, pl):
    got = got.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero((got != RP.pack_results(want)).any(1))
    return len(bad), bad[:4].tolist(), pl[bad[:4]].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


def _assert_sheets(want, sheets):
    """the sheet placements in turn: a fit that overlaps, a drop that lands after moving, a sweep that is stopped"""
    for k, i in enumerate(sheets):
        if k % 3 == 0:
            assert want[i, 0] > 3 and want[i, 3] == 0, (i, want[i])
        else:
            assert want[i, 3] == RP.BLOCKED and want[i, 1] != 0 and want[i, 2] > 0, (i, want[i])


def _sheet_tasks(piece, pl_row, vox, lanes=64):
    """the tasks of a sheet placement whose rows overlap the world at the origin"""
    _, py, pz = np.nonzero(piece & RP.window(vox, pl_row[1:4], piece.shape))
    return set(((py + piece.shape[1] * pz) // lanes).tolist())


def test_placements_on_the_second_grid_axis(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    vox, pieces = np.asarray(F.piece_world()), F.piece_table(F.SHEET_EDGE)
    assert F.place_shape([p.shape for p in pieces]) == (64, 16384)
    pl = F.grid_y_batch(F.SHEET_EDGE)
    want = F.sheet_reference(vox, pieces, pl)
    # reached: sheets on both sides of workgroup 2^20 whose sums and minima meet over many tasks, and the last task's row
    _assert_sheets(want, F.GRID_Y_SHEETS)
    per = 64 * 16384 // 256
    assert [i for i in F.GRID_Y_SHEETS if i * per >= caps["grid_2d_x"]][:2] == [256, 257] and 255 in F.GRID_Y_SHEETS
    assert len(_sheet_tasks(pieces[0], pl[254], vox)) > 3 and len(_sheet_tasks(pieces[0], pl[257], vox)) > 3
    assert pieces[0][0, -1, -1] and want[256:, 3].any() and want[256:, 0].any()
    ctx = _ctx(vx, vxo, vox, F.PIECE_WORLD[3])
    try:
        dev = [vx.Piece(p) for p in pieces]
        bad = _mismatch(_place(vx, torch, ctx, dev, pl), want, pl)
        assert bad[0] == 0, bad
        # the last row of the sheet alone: the last task of a placement on the second grid row
        last = np.zeros_like(pieces[0])
        last[0, -1, -1] = True
        pl2 = pl.copy()
        pl2[299] = [0, 50, 33 - (F.SHEET_EDGE - 1), 50 - (F.SHEET_EDGE - 1), 1, -9]
        want2 = F.sheet_reference(vox, [last] + pieces[1:], pl2)
        assert want2[299].tolist() == [0, -1, 1, 1]
        bad = _mismatch(_place(vx, torch, ctx, [vx.Piece(last)] + dev[1:], pl2), want2, pl2)
        assert bad[0] == 0, bad
    finally:
        ctx.close()


def test_a_batch_cut_into_three_launches(eng, vxo):
    vx, torch = eng
    caps = F.read_caps()
    vox, pieces = np.asarray(F.piece_world()), F.piece_table(F.SHEET_EDGE)
    most = F.place_most([p.shape for p in pieces], caps)
    pl, cuts = F.cut_batch(F.SHEET_EDGE, most)
    want = F.sheet_reference(vox, pieces, pl)
    # reached: three launches; blocked placements beside each cut; no shift by whole rows maps the results, or those of the
    # second or third launch, onto rows of the batch, nor the placements; every launch holds blocked and moved placements
    assert len(pl) == F.CUT_N == 2 * most + 7 and cuts.tolist() == [most - 1, most, 2 * most - 1, 2 * most]
    assert (want[cuts, 3] == RP.BLOCKED).all() and (want[1:] != want[:-1]).any(1).all()
    assert F.no_shift_maps_onto_itself(want) and F.no_shift_maps_onto_itself(want, most) and F.no_shift_maps_onto_itself(want, 2 * most)
    assert F.no_shift_maps_onto_itself(pl)
    assert sorted({int(i) // most for i in np.flatnonzero(want[:, 3] == RP.INVALID)}) == [0, 1, 2]
    sheets = np.flatnonzero(pl[:, 0] == 0)
    assert [int(i) // most for i in sheets] == [0, 1, 2]
    _assert_sheets(want, sheets)
    assert all(want[most * k:most * (k + 1), 3].any() and want[most * k:most * (k + 1), 1].any() for k in range(3))
    ctx = _ctx(vx, vxo, vox, F.PIECE_WORLD[3])
    try:
        dev = [vx.Piece(p) for p in pieces]
        whole = _place(vx, torch, ctx, dev, pl)
        bad = _mismatch(whole, want, pl)
        assert bad[0] == 0, bad
        for at in (most, 1000):
            parts = torch.cat([_place(vx, torch, ctx, dev, pl[:at]), _place(vx, torch, ctx, dev, pl[at:])])
            assert torch.equal(parts, whole), at
    finally:
        ctx.close()


def test_more_placements_than_init_lanes(eng, vxo):
    """65536 x 256 + 300 placements of the one-voxel piece through vxrt_place_pieces itself, the results pre-filled: every
    row equals the tiled results of the base batch, the words behind the results are untouched"""
    vx, torch = eng
    caps = F.read_caps()
    vox, base = np.asarray(F.piece_world()), F.init_base()
    want = RP.place(vox, [np.ones((1, 1, 1), bool)], base)
    n = caps["place_blocks"] * 256 + F.INIT_EXTRA
    tail = np.arange(caps["place_blocks"] * 256, n) % F.INIT_BASE
    # reached: the placements of the second pass are of several kinds
    assert min(classes(want)) > 0 and (want[tail, 3] == RP.INVALID).any() and (want[tail, 3] == RP.BLOCKED).any() and want[tail, 0].any()
    ctx = _ctx(vx, vxo, vox, F.PIECE_WORLD[3])
    try:
        idx = torch.arange(n, device="cuda") % F.INIT_BASE
        pl = torch.from_numpy(base).cuda()[idx].contiguous()
        expect = torch.from_numpy(RP.pack_results(want).view(np.int32)).cuda()[idx]
        del idx
        res = torch.full((n * 4 + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        bits = torch.ones(1, dtype=torch.int32, device="cuda")
        p = vx.PieceDesc()
        p.d_bits, p.dims, p.reserved = bits.data_ptr(), (C.c_int32 * 3)(1, 1, 1), 0
        assert ctx._L.vxrt_place_pieces(ctx._h, (vx.PieceDesc * 1)(p), 1, pl.data_ptr(), n, res.data_ptr(), None) == 0
        torch.cuda.synchronize()
        wrong = (res[:n * 4].view(n, 4) != expect).any(1)
        assert not bool(wrong.any()), (int(wrong.sum()), torch.nonzero(wrong)[:4].flatten().tolist())
        assert bool((res[n * 4:] == 0x5A5A5A5A).all())
    finally:
        ctx.close()
