"""World queries on the device at the operand extremes include/vxrt.h admits, bit for bit against the references: box
collision with faces just below and at the 2^24 validity bound; edits with int32-extreme box corners, spheres of radius
2^31 - 1 whose surface crosses the world, and radius 0; stamps and region reads whose box starts near INT32_MIN or runs
past INT32_MAX, two of them reaching the world only after more than 2^30 voxels of row; island boxes at the ends of int32
(empty by construction: they guard against a wrap into the world and against faults); nav boxes whose halo does not fit in
int32 (memset, not read: the workspace is dirtied by a field inside the world first) and the last ones whose halo does.

Then the launch-cap cases of tests/query_limit_cases.py, each with an assertion from the call's own outputs that it
reached its path: a nav window of the bench world with 4096 goals (repeats 256 apart) and more than 2^20 path starts, the
snake corridor at max_steps = 65535 against its closed form, an island box of 2^24 region words and a 256^3 parity
checkerboard, and calls of 1024 edit ops and 1024 stamps whose last whole-brick cover sits at 63, 64, 255, 256 and 1023."""
import numpy as np
import pytest

from oracle import ref_edit, ref_region, vxo_edit
from tests import query_limit_cases as Q
from tests import ref_collide, ref_islands, ref_nav
from tests.helpers import assert_batch, assert_frames, assert_tables, eng, float_bits, gen_dense, new_ctx, upload

pytestmark = pytest.mark.gpu
BOX, SPHERE = 0, 1
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
R31 = 2 ** 31 - 1
YXZ, XYZ, ZYX = (1, 0, 2), (0, 1, 2), (2, 1, 0)


def _terrain(vxo, edge=128):
    dense = gen_dense(vxo, vxo.GEN_INT_TERRAIN, edge, edge, edge)
    return dense, vxo_edit.voxels_from_dense(dense, edge, edge, edge)


# ---- collision
DELTAS = (64.0, -64.0, 0.5, -0.5, 0.0, -0.0, 1e-45, -1e-45, 3e-39)
FACES = (2.0 ** 24 - 1, 2.0 ** 24 - 2, 2.0 ** 24)


def _bound_bodies():
    """on each axis, a body whose far face (or near face, mirrored) is at +-F for F in FACES, three voxels and one voxel
    thick, with every delta of DELTAS on that axis and others on the two other axes; and bodies at the bound on all axes"""
    rows = []
    for a in range(3):
        for F in FACES:
            for sign in (1.0, -1.0):
                for k, dl in enumerate(DELTAS):
                    d = [DELTAS[(k + 3) % len(DELTAS)], DELTAS[(k + 5) % len(DELTAS)], DELTAS[(k + 7) % len(DELTAS)]]
                    d[a] = dl
                    for thick in (3.0, 1.0):
                        lo, hi = [3.0, 4.0, 5.0], [6.0, 7.5, 8.0]
                        lo[a], hi[a] = (F - thick, F) if sign > 0 else (-F, -F + thick)
                        rows.append(lo + hi + d)
    for F in FACES:
        for k, dl in enumerate(DELTAS):
            rows.append([F - 2.0] * 3 + [F] * 3 + [dl, -dl, DELTAS[(k + 1) % len(DELTAS)]])
            rows.append([-F] * 3 + [-F + 2.0] * 3 + [-dl, dl, DELTAS[(k + 2) % len(DELTAS)]])
    return np.asarray(rows, np.float32)


def test_bodies_at_the_coordinate_bound(eng, vxo):
    vx, torch = eng
    size = (64, 64, 64)
    vox = np.random.default_rng(24).random(size) < 0.05
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        b = _bound_bodies()
        ok = ref_collide.valid(b)
        assert ok.sum() > 100 and (~ok).sum() > 100        # both sides of the bound
        db = torch.from_numpy(b).cuda()
        for order in (YXZ, XYZ, ZYX):
            lohi, flags = ctx.move_boxes(db, order)
            wl, wf = ref_collide.move_boxes(vox, b, order)
            assert np.array_equal(float_bits(lohi.cpu().numpy()), float_bits(wl)), order
            assert np.array_equal(flags.cpu().numpy().view(np.uint32), wf), order
            moved = ok & (float_bits(wl) != float_bits(b[:, :6])).any(1)
            assert moved.sum() > 100                         # the valid bodies near the bound do move
        hl, hf = ctx.move_boxes(b)
        wl, wf = ref_collide.move_boxes(vox, b)
        assert np.array_equal(float_bits(hl), float_bits(wl)) and np.array_equal(hf, wf)
        counts, flags = ctx.overlap_boxes(db)
        wc, wo = ref_collide.overlap_boxes(vox, b)
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), wc)
        assert np.array_equal(flags.cpu().numpy().view(np.uint32), wo)
    finally:
        ctx.close()


# ---- edits
def _extreme_ops():
    a = int(R31 / 2 ** 0.5) - 64        # (-a, -a, 64): the surface passes near x + y = 128
    b = int(R31 / 2 ** 0.5) + 100       # (b, b, 64): the surface passes near x + y = 200
    return [
        (SPHERE, 0, (INT32_MAX, 70, 70), (R31, 0, 0)),                         # clears x >= 1, and (0, 70, 70)
        (SPHERE, 1, (100, 61 - 2 ** 31, 30), (R31, 0, 0)),                     # sets y <= 59, and (100, 60, 30)
        (BOX, 0, (INT32_MIN, 40, INT32_MIN), (INT32_MAX, 41, INT32_MAX)),      # clears the slab y = 40 .. 41
        (SPHERE, 0, (-a, -a, 64), (R31, 0, 0)),
        (SPHERE, 1, (b, b, 64), (R31, 0, 0)),
        (SPHERE, 1, (-R31, 70, 70), (R31, 0, 0)),                              # sets (0, 70, 70) alone
        (SPHERE, 0, (INT32_MAX, INT32_MAX, INT32_MAX), (R31, 0, 0)),           # squares summing to ~3 * 2^62: nothing
        (SPHERE, 1, (INT32_MIN, INT32_MIN, INT32_MIN), (R31, 0, 0)),           # clipped away
        (BOX, 1, (INT32_MAX, 0, 0), (INT32_MAX, 10, 10)),                      # outside
        (BOX, 1, (5, 5, 5), (INT32_MIN, 9, 9)),                                # empty: a > b
        (SPHERE, 1, (10, 100, 10), (0, 0, 0)),                                 # radius 0: one voxel
        (SPHERE, 0, (64, 30, 64), (0, 0, 0)),
        (BOX, 1, (INT32_MIN, INT32_MIN, 100), (INT32_MAX, 3, INT32_MAX)),
    ]


def test_edits_with_int32_extreme_operands(eng, vxo):
    vx, torch = eng
    X = 128
    dense, vox = _terrain(vxo)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(dense, X, X, X, 16))
        ops = _extreme_ops()
        ctx.edit_voxels([vx.EditBox(a, b, v) if k == BOX else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])
        dense = vxo_edit.apply_edits(dense, X, X, X, ops)
        want = vxo_edit.voxels_from_dense(dense, X, X, X)
        assert np.array_equal(want, ref_edit.apply_edits(vox, ops))          # the two restatements agree
        # the one-voxel reaches of the radius-(2^31 - 1) spheres, and the radius-0 ones
        assert want[0, 70, 70] and not want[1, 70, 70] and want[100, 60, 30] and not want[101, 60, 30]
        assert want[10, 100, 10] and not want[64, 30, 64]
        w = vxo.World.from_dense(dense, X, X, X, 16)
        assert_tables(ctx, w)
        assert np.array_equal(ctx.read_region_host((0, 0, 0), (X, X, X)), want)
        assert_frames(vx, ctx, torch, vxo, w, cams="AB", variants=(4,))
        assert_batch(ctx, w)
    finally:
        ctx.close()


# ---- stamps and region reads
FAR = 2 ** 31 - 200    # a row from x = -FAR (INT32_MIN + 200) reaches world x = 0 after FAR voxels
LONG = 2 ** 30 + 40


def _row_words(vx, torch, n, rows, at, tails, fill):
    """device region words of `rows` rows of n voxels each: every bit `fill` but bits [at, at + len(tail)) of row r =
    tails[r]"""
    wpr = (n + 31) // 32
    words = torch.full((rows * wpr,), -1 if fill else 0, dtype=torch.int32, device="cuda")
    w0, s = divmod(at, 32)
    for r, tail in enumerate(tails):
        packed = vx.pack_region(np.concatenate([np.full(s, fill, bool), tail])[:, None, None])
        assert w0 + len(packed) <= wpr
        words[r * wpr + w0:r * wpr + w0 + len(packed)] = torch.from_numpy(packed.view(np.int32)).cuda()
    return words


def _row_bits(words, n, rows, at, count):
    """bits [at, at + count) of each of `rows` region rows of n voxels (device words), and whether every bit of each row
    before bit at is 0"""
    wpr = (n + 31) // 32
    w0, s = divmod(at, 32)
    out, zero = [], []
    for r in range(rows):
        row = words[r * wpr:(r + 1) * wpr]
        tail = row[w0:].cpu().numpy().view(np.uint32)
        bits = np.unpackbits(tail.view(np.uint8), bitorder="little").astype(bool)
        zero.append(int((row[:w0] != 0).sum().item()) == 0 and not bits[:s].any())
        out.append(bits[s:s + count])
    return np.stack(out), all(zero)


def test_stamps_and_reads_at_the_ends_of_int32(eng, vxo):
    vx, torch = eng
    X = 128
    dense, vox = _terrain(vxo)
    rng = np.random.default_rng(31)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(dense, X, X, X, 16))
        # two rows from x = -LONG (REPLACE, 100 voxels in the world) and one from x = -FAR (UNION, 60 voxels in the world);
        # the bits before the world are all set and must be ignored
        long_tails = [rng.random(100) < 0.5 for _ in range(2)]
        far_tail = rng.random(60) < 0.5
        long_words = _row_words(vx, torch, LONG + 100, 2, LONG, long_tails, True)
        far_words = _row_words(vx, torch, FAR + 60, 1, FAR, [far_tail], True)
        ones = lambda d: np.ones(d, bool)
        near = rng.random((20, 10, 12)) < 0.4
        stamps = [  # (origin, device words or bool grid, dims, mode, the part in the world for the reference)
            ((INT32_MAX - 9, 0, 0), ones((32, 16, 16)), None, vx.STAMP_REPLACE, None),    # runs past INT32_MAX
            ((INT32_MIN, 3, 5), ones((64, 1, 1)), None, vx.STAMP_REPLACE, None),          # starts at INT32_MIN
            ((-LONG, 6, 9), long_words, (LONG + 100, 2, 1), vx.STAMP_REPLACE,
             ((0, 6, 9), np.stack(long_tails, 1)[:, :, None])),
            ((-FAR, 9, 11), far_words, (FAR + 60, 1, 1), vx.STAMP_UNION, ((0, 9, 11), far_tail[:, None, None])),
            ((10, INT32_MAX - 3, 7), ones((8, 8, 8)), None, vx.STAMP_SUBTRACT, None),
            ((3, 4, INT32_MIN), ones((4, 4, 4)), None, vx.STAMP_REPLACE, None),
            ((-5, 50, 60), near, None, vx.STAMP_REPLACE, None),
        ]
        ctx.edit_stamps([vx.Stamp(o, bits, mode, dims) for o, bits, dims, mode, _ in stamps])
        want = ref_region.apply_stamps(vox, [(part[0], part[1], mode) if part else (o, bits, mode)
                                             for o, bits, dims, mode, part in stamps])
        assert not np.array_equal(want[:100, 6:8, 9], vox[:100, 6:8, 9])    # the long rows reached the world
        w = vxo.World.from_voxels(want, 16)
        assert_tables(ctx, w)
        assert_frames(vx, ctx, torch, vxo, w, cams="AB", variants=(4,))
        assert_batch(ctx, w)
        # reads of the same rows after the stamps: 32 voxels before the world and the row's part in it
        for o, rows, n in [((-LONG, 6, 9), 2, LONG + 100), ((-FAR, 9, 11), 1, FAR + 60)]:
            words = ctx.read_region(o, (n, rows, 1))
            assert words.numel() == rows * ((n + 31) // 32)
            at = -o[0] - 32
            bits, zero = _row_bits(words, n, rows, at, n - at)
            assert zero
            row = np.zeros((rows, n - at), bool)
            row[:, 32:] = want[:n - at - 32, o[1]:o[1] + rows, o[2]].T
            assert np.array_equal(bits, row), o
        for o, d in [((INT32_MAX - 9, 0, 0), (32, 16, 16)), ((INT32_MIN, 3, 5), (64, 1, 1)), ((10, INT32_MAX - 3, 7), (8, 8, 8)),
                     ((INT32_MIN, INT32_MIN, INT32_MIN), (40, 33, 70)),
                     ((INT32_MAX - 40, INT32_MAX - 40, INT32_MAX - 40), (100, 100, 3)), ((-60, 100, 120), (300, 40, 20))]:
            assert np.array_equal(ctx.read_region_host(o, d), ref_region.read_region(want, o, d)), o
    finally:
        ctx.close()


# ---- islands and nav
ISL_BOXES = [((INT32_MIN, 0, 0), (64, 40, 33)), ((0, INT32_MIN, 0), (40, 64, 40)), ((7, 3, INT32_MAX - 70), (50, 30, 70)),
             ((INT32_MAX - 33, INT32_MAX - 33, INT32_MAX - 33), (33, 33, 33))]
# boxes whose halo ([o[1] - 1, o[1] + d[1] + height - 1) in y, [o, o + d + width - 1) in x and z) leaves int32 ...
NAV_HALO_OUT = [((0, INT32_MIN, 0), (8, 8, 8), (1, 2, 1, 3)), ((INT32_MAX - 8, 0, 0), (8, 8, 8), (8, 2, 1, 3)),
                ((3, 1, INT32_MAX - 40), (16, 8, 40), (2, 3, 0, 1)), ((5, INT32_MAX - 16, 2), (8, 16, 8), (1, 32, 8, 32))]
# ... and the last boxes whose halo fits: a read at y = INT32_MIN, and halo ends at exactly INT32_MAX
NAV_HALO_FITS = [((0, INT32_MIN + 1, 0), (8, 8, 8), (1, 2, 1, 3)), ((INT32_MAX - 15, 0, 0), (8, 8, 8), (8, 2, 1, 3)),
                 ((INT32_MAX - 8, 0, 0), (8, 8, 8), (1, 2, 1, 3))]


def _halo_fits(o, d, agent):
    w, h = agent[0], agent[1]
    return o[1] - 1 >= INT32_MIN and max(o[0] + d[0] + w - 1, o[1] + d[1] + h - 1, o[2] + d[2] + w - 1) <= INT32_MAX


def test_island_and_nav_boxes_at_the_ends_of_int32(eng, vxo):
    vx, torch = eng
    vox = np.random.default_rng(32).random((64, 64, 64)) < 0.2
    vox[:, 0, :] = True
    vox[:, 20:, :] = False                                   # room above y = 20 for the tallest agent
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, 8))
        for o, d in ISL_BOXES:
            assert max(o[k] + d[k] for k in range(3)) <= INT32_MAX
            for anchors in (ref_islands.FACES | ref_islands.FLOOR, 0):
                r = ctx.find_islands(o, d, anchors, labels=True)
                want = ref_islands.fast(ref_region.read_region(vox, o, d), o, anchors)
                assert tuple(r.summary) == want["summary"] == (0, 0, 0), (o, anchors)
                assert int(r.floating.count_nonzero()) == 0 and int(r.labels.count_nonzero()) == 0 and len(r.table) == 0
        assert all(not _halo_fits(*b) for b in NAV_HALO_OUT) and all(_halo_fits(*b) for b in NAV_HALO_FITS)
        for o, d, agent in NAV_HALO_OUT + NAV_HALO_FITS:
            assert max(o[k] + d[k] for k in range(3)) <= INT32_MAX
            # a field of the same dims and agent inside the world first: the caching allocator hands its workspace (its
            # halo bits included) to the call below, so a halo that is neither memset nor read would show as nodes
            dirty = ctx.nav_field((2, 20, 3), d, [], vx.NavAgent(*agent))
            assert dirty.summary.nodes > 0
            del dirty
            goals = [o, (o[0] + 1, o[1] + 1, o[2] + 1), (o[0] + d[0] - 1, o[1] + d[1] - 1, o[2] + d[2] - 1), (1, 1, 1)]
            r = ctx.nav_field(o, d, goals, vx.NavAgent(*agent))
            want = ref_nav.nav_field(vox, o, d, agent, goals)
            assert tuple(r.summary)[:6] == want["summary"] and want["summary"][:4] == (0, 0, len(goals), 0), (o, agent)
            assert r.summary.tiles_total == -(-d[0] // 32) * -(-d[1] // 16) * -(-d[2] // 16)
            assert int(r.walkable.count_nonzero()) == 0
            assert np.array_equal(r.next.cpu().numpy().reshape(d[::-1]).transpose(2, 1, 0), want["next"])
            assert np.array_equal(r.dist.cpu().numpy().view(np.uint32).reshape(d[::-1]).transpose(2, 1, 0), want["dist"])
    finally:
        ctx.close()


# ==== launch-cap cases (tests/query_limit_cases.py) ==================================================================
def _grid(t, dims, dtype):
    return t.cpu().numpy().view(dtype).reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)


def _nav_want(world, origin, dims, agent, goals, max_dist=1 << 24):
    f = ref_nav.nav_field_scipy if ref_nav.have_scipy() else ref_nav.nav_field
    return f(world, origin, dims, agent, goals, max_dist)


def _assert_field(vx, r, want, dims, caps):
    assert tuple(r.summary)[:6] == want["summary"], (tuple(r.summary), want["summary"])
    assert r.summary.tiles_total == Q.nav_tiles(dims, caps)
    assert np.array_equal(r.walkable.cpu().numpy().view(np.uint32), vx.pack_region(want["walkable"]))
    assert np.array_equal(_grid(r.dist, dims, np.uint32), want["dist"])
    assert np.array_equal(_grid(r.next, dims, np.uint8), want["next"])


def test_nav_window_4096_goals_and_a_million_paths(eng):
    vx, torch = eng
    caps = Q.read_caps()
    sh = Q.NAV_WINDOW.shape
    (ox, oz), d, agent = sh["corner"], sh["dims"], sh["agent"]
    ctx = vx.Context(0)
    try:
        ctx.build_world(vx.GEN_PERLIN_REF, *sh["world"])
        tops = []
        for k in range(0, d[2], 128):
            col = ctx.read_region_host((ox, 0, oz + k), (d[0], 512, 1))[:, :, 0]
            tops.append(np.where(col.any(1), 511 - np.argmax(col[:, ::-1], axis=1), 0))
        y0 = max(int(np.median(np.concatenate(tops))) - d[1] // 2, 1)
        o, shift = (ox, y0, oz), np.asarray((ox, y0 - 1, oz))
        world = ctx.read_region_host(tuple(shift), (d[0], d[1] + agent[1], d[2]))  # a width-1 agent's halo, cell 0 at shift
        free, sup = ref_nav.free_supported(world, (0, 1, 0), d, agent)
        walk = free & sup
        nodes = np.argwhere(walk)
        assert len(nodes) > 100000
        rng = np.random.default_rng(4096)
        cells = np.stack([rng.integers(0, n, 20000) for n in d], 1)
        non = cells[~walk[tuple(cells.T)]]
        far = np.stack([rng.integers(-40, n + 40, 20000) for n in d], 1)
        far = far[((far < 0) | (far >= np.asarray(d))).any(1)]
        base = np.concatenate([nodes[rng.choice(len(nodes), 2000, replace=False)], non[:600], far[:472]])
        base = base[rng.permutation(len(base))]
        assert len(base) == sh["repeat_from"]
        goals = list(base)
        for i in range(sh["repeat_from"], sh["goals"]):
            goals.append(goals[i - sh["repeat_stride"]])   # the same goal again, in another workgroup of k_nav_goals
        goals = np.asarray(goals) + np.asarray(o)
        r = ctx.nav_field(o, d, goals, vx.NavAgent(*agent))
        want = _nav_want(world, (0, 1, 0), d, agent, goals - shift)
        _assert_field(vx, r, want, d, caps)
        s = r.summary
        assert s.goals_used + s.goals_ignored == len(goals) and s.goals_used > 2000 and s.goals_ignored > 1000
        # max_dist 12: the same field cut at 12 (a cell's next depends on the cells one level down only), few levels over
        # many tiles each
        cut = ctx.nav_field(o, d, goals, vx.NavAgent(*agent), sh["max_dist"])
        keep = want["dist"] <= sh["max_dist"]
        cw = dict(walkable=want["walkable"], dist=np.where(keep, want["dist"], ref_nav.UNREACHED).astype(np.uint32),
                  next=np.where(keep, want["next"], ref_nav.NONE).astype(np.uint8))
        mx = int(cw["dist"][keep].max())
        cw["summary"] = tuple(want["summary"][:3]) + (int(keep.sum()), mx, mx + 1)
        _assert_field(vx, cut, cw, d, caps)
        assert cut.summary.tile_visits > caps["nav_level_groups"] * cut.summary.levels, cut.summary
        # paths from more than 2^20 starts: nodes, cells of B that are not nodes, cells outside B
        ps = Q.NAV_PATHS.shape
        starts = np.concatenate([nodes[rng.integers(0, len(nodes), ps["nodes"])], non[:ps["non_nodes"]],
                                 far[:ps["outside"]]]) + np.asarray(o)
        assert len(starts) == (1 << 20) + 4096 + 8192
        starts = starts[rng.permutation(len(starts))].astype(np.int32)
        ms = ps["max_steps"]
        p = r.paths(starts, ms, cells=True)
        _, l, st = Q.decode_paths_np(want["next"], o, agent, starts, ms, cells=False)
        assert np.array_equal(p.lengths.cpu().numpy(), l) and np.array_equal(p.status.cpu().numpy(), st)
        tail = np.arange(caps["nav_paths_blocks"] * 256, len(starts))      # the grid-stride's second pass
        assert (l[tail] > 0).sum() > 1000
        assert set(st[tail].tolist()) == {ref_nav.AT_GOAL, ref_nav.NO_PATH, ref_nav.TRUNCATED, ref_nav.OUTSIDE}
        sub = np.concatenate([np.arange(4096), tail])
        c, _, _ = Q.decode_paths_np(want["next"], o, agent, starts[sub], ms)
        assert np.array_equal(p.cells.cpu().numpy()[sub], c)
    finally:
        ctx.close()


def test_snake_corridor_65535_moves(eng, vxo):
    vx, torch = eng
    caps = Q.read_caps()
    sh = Q.NAV_SNAKE.shape
    X, Z, agent = sh["X"], sh["Z"], sh["agent"]
    snake = ref_nav.snake_world(X, Z)
    vox = np.zeros((X, sh["height"], Z), bool)
    vox[:, :snake.shape[1]] = snake
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(vox, sh["factor"]))
        d = snake.shape
        r = ctx.nav_field((0, 0, 0), d, [(0, 1, 0)], vx.NavAgent(*agent))
        dist, nxt, path = Q.snake_field(X, Z, d[1], agent)
        free, sup = ref_nav.free_supported(vox, (0, 0, 0), d, agent)
        n = len(path)
        assert tuple(r.summary)[:6] == (int((free & sup).sum()), 1, 0, n, n - 1, n)
        assert np.array_equal(r.walkable.cpu().numpy().view(np.uint32), vx.pack_region(free & sup))
        assert np.array_equal(_grid(r.dist, d, np.uint32), dist) and np.array_equal(_grid(r.next, d, np.uint8), nxt)
        ms = caps["nav_max_steps"]
        starts = np.asarray([[path[i][0], 1, path[i][1]] for i in (ms, ms + 1, n - 1)], np.int32)
        p = r.paths(starts, ms)
        c, l, st = Q.decode_paths_np(nxt, (0, 0, 0), agent, starts, ms)
        assert np.array_equal(p.lengths.cpu().numpy(), l) and np.array_equal(p.status.cpu().numpy(), st)
        assert l.tolist() == [ms] * 3 and st.tolist() == [ref_nav.AT_GOAL, ref_nav.TRUNCATED, ref_nav.TRUNCATED]
        got = p.cells.cpu().numpy()
        assert np.array_equal(got, c) and np.array_equal(got[0][:, [0, 2]], path[ms::-1])
    finally:
        ctx.close()


def test_islands_thin_box_past_the_output_cap(eng, vxo):
    vx, torch = eng
    caps = Q.read_caps()
    sh = Q.ISL_THIN.shape
    o, d = sh["origin"], sh["dims"]
    ctx = vx.Context(0)
    try:
        ctx.build_world(vxo.GEN_INT_TERRAIN, *sh["world"], sh["factor"])
        bits = np.random.default_rng(1 << 24).random(d) < sh["density"]
        words = bits[0].T.reshape(-1).astype(np.uint32)           # dims[0] = 1: one word per row, rows y fastest
        dev = torch.from_numpy(words.view(np.int32)).cuda()
        ctx.edit_stamps([vx.Stamp(o, dev, vx.STAMP_REPLACE, d)])
        assert torch.equal(ctx.read_region(o, d), dev)
        cap = caps["isl_output_blocks"] * 4 * caps["isl_pairs_per_wave"] * 2
        for anchors, labels in [(0, True), (ref_islands.Y_LO | ref_islands.Z_HI, False),
                                (ref_islands.FLOOR | ref_islands.Z_LO, False)]:
            r = ctx.find_islands(o, d, anchors, labels=labels, max_islands=sh["max_islands"])
            want = ref_islands.fast(bits, o, anchors)
            assert tuple(r.summary) == want["summary"], anchors
            fl = r.floating.cpu().numpy().view(np.uint32)
            assert fl.size > cap and np.array_equal(fl, want["floating"][0].T.reshape(-1).astype(np.uint32))
            assert fl[cap:].any()                                  # island words in the grid-stride's second pass
            if labels:
                assert np.array_equal(r.labels.cpu().numpy().view(np.uint32), want["labels"][0].T.reshape(-1))
            assert np.array_equal(ref_islands.table_rows(r.table), want["table"][:sh["max_islands"]])
    finally:
        ctx.close()


def test_islands_checkerboard_every_voxel_its_own_island(eng, vxo):
    vx, torch = eng
    sh = Q.ISL_CHECKER.shape
    d = sh["dims"]
    ctx = vx.Context(0)
    try:
        upload(ctx, vxo.World.from_voxels(Q.checkerboard(d), sh["factor"]))
        for anchors, mx in zip((0, ref_islands.FACES), sh["max_islands"]):
            r = ctx.find_islands((0, 0, 0), d, anchors, max_islands=mx)
            summary, floating, ids, lo = Q.checker_islands(d, (0, 0, 0), anchors)
            assert tuple(r.summary) == summary and summary[1] == summary[2] > 0, anchors  # one voxel per island
            k = min(summary[1], mx)
            t = r.table
            assert len(t) == k and np.array_equal(t["id"], ids[:k]) and (t["voxels"] == 1).all()
            assert np.array_equal(t["lo"], lo[:k]) and np.array_equal(t["hi"], lo[:k] + 1)
            assert np.array_equal(r.floating.cpu().numpy().view(np.uint32), vx.pack_region(floating))
        assert summary[1] > mx                                     # the truncated table kept the true count
    finally:
        ctx.close()


COVER_BRICKS = [(1, 1, 1), (2, 3, 4), (5, 2, 6), (6, 6, 1), (3, 5, 3)]  # brick j is covered last at COVER_AT[j]


def _place(ops, rng, items, lo, hi):
    """put each item at a free index in [lo, hi)"""
    if not items:
        return
    free = [i for i in range(lo, hi) if ops[i] is None]
    for i, it in zip(rng.choice(free, len(items), replace=False), items):
        ops[int(i)] = it


def _fill(ops, rng, make):
    for i in range(len(ops)):
        if ops[i] is None:
            ops[i] = make()


def _ops_1024(rng, f=16, X=128):
    ops = [None] * Q.EDIT_1024.shape["ops"]

    def partial(b):
        lo = [v * f + int(rng.integers(0, f - 6)) for v in b]
        val = int(rng.integers(0, 2))
        if rng.random() < 0.5:
            return (BOX, val, lo, [v + int(rng.integers(0, 5)) for v in lo])
        return (SPHERE, val, [v + 2 for v in lo], (int(rng.integers(0, 4)), 0, 0))

    def small():
        lo = [int(rng.integers(-4, X)) for _ in range(3)]
        if rng.random() < 0.5:
            return (BOX, int(rng.integers(0, 2)), lo, [v + int(rng.integers(0, 5)) for v in lo])
        return (SPHERE, int(rng.integers(0, 2)), lo, (int(rng.integers(0, 4)), 0, 0))

    for j, (k, b) in enumerate(zip(Q.COVER_AT, COVER_BRICKS)):
        lo, hi, val = [v * f for v in b], [v * f + f - 1 for v in b], (j + 1) % 2
        ops[k] = ((BOX, val, [v - j for v in lo], [v + j for v in hi]) if j % 2 == 0 else
                  (SPHERE, val, [v + f // 2 for v in lo], (f - 2, 0, 0)))  # a ball holding the brick's eight corners
        ops[k // 2] = (BOX, 1 - val, lo, hi)                                 # an earlier cover, of the other value
    for j, (k, b) in enumerate(zip(Q.COVER_AT, COVER_BRICKS)):
        _place(ops, rng, [partial(b) for _ in range(10)], 0, k)             # before the cover: overridden
        _place(ops, rng, [partial(b) for _ in range(300 if j == 0 else 20 if k < 1023 else 0)], k + 1, len(ops))
    _fill(ops, rng, small)
    return ops


def _edit(vx, ctx, ops):
    return ctx.edit_voxels([vx.EditBox(a, b, v) if k == BOX else vx.EditSphere(a, b[0], v) for k, v, a, b in ops])


def test_1024_edit_ops_with_covers_past_every_chunk(eng, vxo):
    vx, torch = eng
    X, f = 128, 16
    dense, vox = _terrain(vxo)
    rng = np.random.default_rng(1024)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_dense(dense, X, X, X, f))
        ops = _ops_1024(rng)
        later = [(k, int(rng.integers(0, 2)), [v * f + int(rng.integers(0, f - 4)) for v in b], None)
                 for k, b in [(int(rng.integers(0, 2)), COVER_BRICKS[int(rng.integers(0, 5))]) for _ in range(200)]]
        later = [(k, v, a, [x + 3 for x in a] if k == BOX else (3, 0, 0)) for k, v, a, _ in later]
        for call in (ops, later):
            st = _edit(vx, ctx, call)
            dense = vxo_edit.apply_edits(dense, X, X, X, call)
            want = vxo_edit.voxels_from_dense(dense, X, X, X)
            vox = ref_edit.apply_edits(vox, call)
            assert np.array_equal(want, vox) and st.bricks_touched >= len(COVER_BRICKS)
            w = vxo.World.from_dense(dense, X, X, X, f)
            assert_tables(ctx, w)
            assert_frames(vx, ctx, torch, vxo, w, cams="A", variants=(4,))
            assert_batch(ctx, w)
            if call is ops:  # the brick whose cover is op 1023 is that op's value throughout, whatever came before
                b = [v * f for v in COVER_BRICKS[4]]
                assert ctx.read_region_host(b, (f, f, f)).all()
                assert not want[16:32, 16:32, 16:32].all() and want[16:32, 16:32, 16:32].any()  # brick 0: partial ops after
    finally:
        ctx.close()


def _stamps_1024(rng, f=16, X=128):
    st = [None] * Q.STAMP_1024.shape["stamps"]

    def partial(b):
        o = tuple(v * f + int(rng.integers(0, f - 6)) for v in b)
        return (o, rng.random(tuple(int(rng.integers(1, 6)) for _ in range(3))) < 0.5, int(rng.integers(0, 3)))

    def small():
        o = tuple(int(rng.integers(-4, X)) for _ in range(3))
        return (o, rng.random(tuple(int(rng.integers(1, 6)) for _ in range(3))) < 0.5, int(rng.integers(0, 3)))

    for j, (k, b) in enumerate(zip(Q.COVER_AT, COVER_BRICKS)):
        lo = tuple(v * f - j for v in b)
        st[k] = (lo, rng.random((f + 2 * j,) * 3) < 0.5, ref_region.REPLACE)
        st[k // 2] = (tuple(v * f for v in b), rng.random((f, f, f)) < 0.5, ref_region.REPLACE)
    for j, (k, b) in enumerate(zip(Q.COVER_AT, COVER_BRICKS)):
        _place(st, rng, [partial(b) for _ in range(10)], 0, k)
        _place(st, rng, [partial(b) for _ in range(300 if j == 0 else 20 if k < 1023 else 0)], k + 1, len(st))
    # union and subtract stamps that hold brick 1 whole: they do not cover it (only replace does), the list must go on
    b1 = tuple(v * f - 1 for v in COVER_BRICKS[1])
    _place(st, rng, [(b1, rng.random((f + 2,) * 3) < 0.5, m) for m in (ref_region.UNION, ref_region.SUBTRACT) * 3],
           Q.COVER_AT[1] + 1, Q.COVER_AT[2])
    _fill(st, rng, small)
    return st


def test_1024_stamps_with_covers_past_every_chunk(eng, vxo):
    vx, torch = eng
    X, f = 128, 16
    _, vox = _terrain(vxo)
    rng = np.random.default_rng(2048)
    ctx = new_ctx(vx)
    try:
        upload(ctx, vxo.World.from_voxels(vox, f))
        stamps = _stamps_1024(rng)
        later = [(tuple(v * f + int(rng.integers(0, f - 6)) for v in COVER_BRICKS[int(rng.integers(0, 5))]),
                  rng.random((5, 4, 3)) < 0.5, int(rng.integers(0, 3))) for _ in range(200)]
        for call in (stamps, later):
            st = ctx.edit_stamps([vx.Stamp(o, m, mode) for o, m, mode in call])
            vox = ref_region.apply_stamps(vox, call)
            assert st.bricks_touched >= len(COVER_BRICKS)
            w = vxo.World.from_voxels(vox, f)
            assert_tables(ctx, w)
            assert_frames(vx, ctx, torch, vxo, w, cams="A", variants=(4,))
            assert_batch(ctx, w)
            if call is stamps:  # the brick covered last by stamp 1023 holds that stamp's bits
                o, m, _ = stamps[1023]
                b = [v * f for v in COVER_BRICKS[4]]
                assert np.array_equal(ctx.read_region_host(b, (f, f, f)), m[4:4 + f, 4:4 + f, 4:4 + f])
    finally:
        ctx.close()
