"""The _host twins of the C ABI (include/vxrt.h) against their device entry points on the same arguments, word for word, at
the shapes the other GPU tests leave out: vxrt_place_pieces_host with VXRT_PLACE_MAX_PIECES pieces (the most scratch sections
one call cuts), vxrt_find_islands_host with a table shorter than the islands found and with no table and no labels,
vxrt_extract_surface_host with a capacity below the quad count with and without vertices, vxrt_trace_batch_host with hit and
voxel both NULL and both given, and the optional outputs no other test leaves out of a host call that succeeds: the flags of
the box queries, the distances of a navigation field, the counts of a downsampled region.  Every caller array is longer than what may come back and filled with a sentinel: what lies
behind the rows a call reports must stay untouched.  One 64^3 world with brick edge 8 serves all of them."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers
from tests.helpers import eng, upload

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A
SIZE = (64, 64, 64)


@pytest.fixture(scope="module")
def ctx(eng, vxo):
    vx, torch = eng
    c = vx.Context(0)
    upload(c, helpers.random_voxel_world(vxo, SIZE, 8, 0.05, seed=11))
    yield c
    c.close()


def _i3(*v):
    return (C.c_int32 * 3)(*v)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).cuda()


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _sentinel(n):
    return np.full(n, SENTINEL, np.uint32)


def test_place_pieces_host_with_the_most_pieces(eng, ctx):
    vx, torch = eng
    L, h = ctx._L, ctx._h
    rng = np.random.default_rng(5)
    n_pieces, n = vx.PLACE_MAX_PIECES, 300
    assert n_pieces == 64
    dims = [(1 + k % 33, 1 + k % 3, 1 + k % 4) for k in range(n_pieces)]  # 1 .. 12 rows of one word (two words at 33 wide)
    bits = [rng.integers(0, 2 ** 32, size=(d[0] + 31) // 32 * d[1] * d[2], dtype=np.uint64).astype(np.uint32) for d in dims]
    dev_bits = [_dev(torch, b) for b in bits]
    pl = np.stack([np.arange(n) % n_pieces, rng.integers(-4, 64, n), rng.integers(-4, 64, n), rng.integers(-4, 64, n),
                   rng.integers(0, 3, n), rng.integers(-12, 13, n)], axis=1).astype(np.int32)
    d_pl = _dev(torch, pl)

    def descs(ptrs):
        out = (vx.PieceDesc * n_pieces)()
        for k in range(n_pieces):
            out[k].d_bits, out[k].dims, out[k].reserved = ptrs[k], _i3(*dims[k]), 0
        return out

    d_res = torch.from_numpy(_sentinel(n * 4 + 64).view(np.int32)).cuda()
    assert L.vxrt_place_pieces(h, descs([t.data_ptr() for t in dev_bits]), n_pieces, d_pl.data_ptr(), n, d_res.data_ptr(), None) == 0
    torch.cuda.synchronize()
    res = _sentinel(n * 4 + 64)
    assert L.vxrt_place_pieces_host(h, descs([b.ctypes.data for b in bits]), n_pieces, pl.ctypes.data, n, res.ctypes.data) == 0
    assert np.array_equal(res, _words(d_res))
    assert (res[n * 4:] == SENTINEL).all() and not (res[:n * 4].reshape(n, 4)[:, 3] & vx.PLACED_INVALID).any()
    assert len({int(v) for v in res[:n * 4].reshape(n, 4)[:, 0]}) > 1  # (the pieces meet the world: not all results alike)


@pytest.mark.parametrize("labels,max_islands", [(True, 5), (False, None), (True, 1 << 15)])
def test_find_islands_host_table_rows(eng, ctx, labels, max_islands):
    """max_islands None: no table.  5: fewer rows than islands.  2^15: more rows than islands."""
    vx, torch = eng
    L, h = ctx._L, ctx._h
    o3, d3 = _i3(0, 0, 0), _i3(*SIZE)
    nvox, nw = SIZE[0] * SIZE[1] * SIZE[2], 2 * SIZE[1] * SIZE[2]
    rows = 0 if max_islands is None else max_islands
    work = torch.zeros(int(L.vxrt_islands_workspace_bytes(d3)), dtype=torch.uint8, device="cuda")
    d_float, d_lab = _dev(torch, _sentinel(nw)), _dev(torch, _sentinel(nvox))
    d_tab, d_sum = _dev(torch, _sentinel((rows + 8) * 8)), _dev(torch, _sentinel(3))
    assert L.vxrt_find_islands(h, o3, d3, vx.ISLAND_ANCHOR_FLOOR, work.data_ptr(), d_float.data_ptr(),
                               d_lab.data_ptr() if labels else None, d_tab.data_ptr() if rows else None, rows, d_sum.data_ptr(),
                               None) == 0
    torch.cuda.synchronize()
    fl, lab, tab, summ = _sentinel(nw), _sentinel(nvox), _sentinel((rows + 8) * 8), _sentinel(3)
    assert L.vxrt_find_islands_host(h, o3, d3, vx.ISLAND_ANCHOR_FLOOR, fl.ctypes.data, lab.ctypes.data if labels else None,
                                    tab.ctypes.data if rows else None, rows, summ.ctypes.data) == 0
    assert np.array_equal(summ, _words(d_sum)) and np.array_equal(fl, _words(d_float))
    islands = int(summ[1])
    assert 5 < islands < 1 << 15, islands
    assert np.array_equal(lab, _words(d_lab)) and (lab == SENTINEL).all() != labels
    back = min(islands, rows)
    assert np.array_equal(tab[:back * 8], _words(d_tab)[:back * 8])
    assert (tab[back * 8:] == SENTINEL).all()  # nothing behind the rows that came back, inside max_islands or beyond


@pytest.mark.parametrize("triangles", [True, False])
def test_extract_surface_host_below_the_quad_count(eng, ctx, triangles):
    vx, torch = eng
    L, h = ctx._L, ctx._h
    o3, d3 = _i3(0, 0, 0), _i3(*SIZE)
    work = torch.zeros(int(L.vxrt_surface_workspace_bytes(d3)), dtype=torch.uint8, device="cuda")
    d_sum = _dev(torch, _sentinel(16))
    assert L.vxrt_extract_surface(h, o3, d3, vx.SURF_CAP, work.data_ptr(), None, 0, None, None, d_sum.data_ptr(), None) == 0
    torch.cuda.synchronize()
    quads = int(_words(d_sum)[2])
    cap = quads // 2 + 1
    assert 1 < cap < quads
    nq = cap + 16  # the caller's arrays are longer than the capacity it states
    d_q, d_v, d_t = _dev(torch, _sentinel(nq * 2)), _dev(torch, _sentinel(nq * 12)), _dev(torch, _sentinel(nq * 6))
    assert L.vxrt_extract_surface(h, o3, d3, vx.SURF_CAP, work.data_ptr(), d_q.data_ptr(), cap, d_v.data_ptr() if triangles else None,
                                  d_t.data_ptr() if triangles else None, d_sum.data_ptr(), None) == 0
    torch.cuda.synchronize()
    q, v, t, summ = _sentinel(nq * 2), _sentinel(nq * 12), _sentinel(nq * 6), _sentinel(16)
    assert L.vxrt_extract_surface_host(h, o3, d3, vx.SURF_CAP, q.ctypes.data, cap, v.ctypes.data if triangles else None,
                                       t.ctypes.data if triangles else None, summ.ctypes.data) == 0
    assert np.array_equal(summ, _words(d_sum))
    written = int(summ[3])
    assert written == cap and int(summ[2]) == quads
    for got, dev, per in ((q, d_q, 2), (v, d_v, 12), (t, d_t, 6)):
        back = written * per if triangles or per == 2 else 0
        assert np.array_equal(got[:back], _words(dev)[:back]), per
        assert (got[back:] == SENTINEL).all(), per  # records past `written` (without triangles: all of them) stay untouched
    assert len(np.unique(q[:written * 2])) > 2


@pytest.mark.parametrize("aovs", [False, True])
def test_trace_batch_host_hit_and_voxel(eng, ctx, aovs):
    """hit and voxel both NULL, and both given"""
    vx, torch = eng
    L, h = ctx._L, ctx._h
    n = 300
    o, d = helpers.mixed_rays(SIZE, n, seed=3)
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    d_o, d_d = _dev(torch, o), _dev(torch, d)
    d_pos, d_nrm, d_steps = (_dev(torch, _sentinel(k)) for k in (n * 3 + 8, n * 3 + 8, n + 8))
    d_hit, d_vox = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device="cuda"), _dev(torch, _sentinel(2 * n + 8))
    assert L.vxrt_trace_batch(h, d_o.data_ptr(), d_d.data_ptr(), n, d_pos.data_ptr(), d_nrm.data_ptr(), d_steps.data_ptr(),
                              d_hit.data_ptr() if aovs else None, d_vox.data_ptr() if aovs else None, None, None) == 0
    torch.cuda.synchronize()
    pos, nrm, steps, vox = _sentinel(n * 3 + 8), _sentinel(n * 3 + 8), _sentinel(n + 8), _sentinel(2 * n + 8)
    hit = np.full(n + 8, 0x5A, np.uint8)
    assert L.vxrt_trace_batch_host(h, o.ctypes.data, d.ctypes.data, n, pos.ctypes.data, nrm.ctypes.data, steps.ctypes.data,
                                   hit.ctypes.data if aovs else None, vox.ctypes.data if aovs else None, None) == 0
    for got, dev in ((pos, d_pos), (nrm, d_nrm), (steps, d_steps), (vox, d_vox)):
        assert np.array_equal(got, _words(dev))
    assert np.array_equal(hit, d_hit.cpu().numpy())
    assert (pos[n * 3:] == SENTINEL).all() and (steps[n:] == SENTINEL).all() and (hit[n:] == 0x5A).all()
    assert (vox[:2 * n] == SENTINEL).all() != aovs and (hit[:n] == 0x5A).all() != aovs
    if aovs:
        assert 0 < int(hit[:n].sum()) < n  # some rays hit, some miss


def test_boxes_host_without_flags(eng, ctx):
    """flags_or_null NULL on a call that succeeds: the same lo / hi and counts, and nothing else written"""
    vx, torch = eng
    L, h = ctx._L, ctx._h
    rng = np.random.default_rng(7)
    n = 200
    lo = rng.uniform(0, 60, (n, 3))
    b = np.concatenate([lo, lo + rng.uniform(0.5, 3, (n, 3)), rng.uniform(-3, 3, (n, 3))], axis=1).astype(np.float32)
    order, d_b = _i3(1, 0, 2), _dev(torch, b)
    d_lohi, d_cnt = _dev(torch, _sentinel(n * 6 + 8)), _dev(torch, _sentinel(n + 8))
    assert L.vxrt_move_boxes(h, d_b.data_ptr(), n, order, d_lohi.data_ptr(), None, None) == 0
    assert L.vxrt_overlap_boxes(h, d_b.data_ptr(), n, d_cnt.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    lohi, cnt = _sentinel(n * 6 + 8), _sentinel(n + 8)
    assert L.vxrt_move_boxes_host(h, b.ctypes.data, n, order, lohi.ctypes.data, None) == 0
    assert L.vxrt_overlap_boxes_host(h, b.ctypes.data, n, cnt.ctypes.data, None) == 0
    assert np.array_equal(lohi, _words(d_lohi)) and np.array_equal(cnt, _words(d_cnt))
    assert (lohi[n * 6:] == SENTINEL).all() and (cnt[n:] == SENTINEL).all() and 0 < int((cnt[:n] > 0).sum()) < n


def test_nav_field_host_without_dist(eng, ctx):
    vx, torch = eng
    L, h = ctx._L, ctx._h
    o3, d3, ag = _i3(0, 0, 0), _i3(*SIZE), vx.NavAgent()._c()
    nvox, nw = SIZE[0] * SIZE[1] * SIZE[2], 2 * SIZE[1] * SIZE[2]
    work = torch.zeros(int(L.vxrt_nav_workspace_bytes(d3, C.addressof(ag))), dtype=torch.uint8, device="cuda")
    d_walk, d_sum = _dev(torch, _sentinel(nw)), _dev(torch, _sentinel(8))
    d_next = torch.full((nvox + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    # three goals among the walkable cells, which a first call without goals finds (region layout: x in words, then y, then z)
    assert L.vxrt_nav_field(h, o3, d3, C.addressof(ag), None, 0, 1 << 24, work.data_ptr(), d_walk.data_ptr(), d_next.data_ptr(),
                            None, d_sum.data_ptr(), None) == 0
    torch.cuda.synchronize()
    words = _words(d_walk)
    at = np.flatnonzero(words)[[0, len(np.flatnonzero(words)) // 2, -1]]
    low = [(int(words[w]) & -int(words[w])).bit_length() - 1 for w in at]
    goals = np.asarray([((w % 2) * 32 + k, (w // 2) % SIZE[1], (w // 2) // SIZE[1]) for w, k in zip(at.tolist(), low)], np.int32)
    d_goals = _dev(torch, goals)
    assert L.vxrt_nav_field(h, o3, d3, C.addressof(ag), d_goals.data_ptr(), len(goals), 1 << 24, work.data_ptr(), d_walk.data_ptr(),
                            d_next.data_ptr(), None, d_sum.data_ptr(), None) == 0
    torch.cuda.synchronize()
    walk, nxt, summ = _sentinel(nw), np.full(nvox + 8, 0x5A, np.uint8), _sentinel(8)
    assert L.vxrt_nav_field_host(h, o3, d3, C.addressof(ag), goals.ctypes.data, len(goals), 1 << 24, walk.ctypes.data,
                                 nxt.ctypes.data, None, summ.ctypes.data) == 0
    assert np.array_equal(summ, _words(d_sum)) and np.array_equal(walk, _words(d_walk))
    assert np.array_equal(nxt, d_next.cpu().numpy()) and (nxt[nvox:] == 0x5A).all()
    assert summ[0] > 3 and summ[1] == 3 and summ[3] >= 3  # walkable nodes, every goal one of them and reached


def test_downsample_region_host_without_counts(eng, ctx):
    vx, torch = eng
    L, h = ctx._L, ctx._h
    shift, dims = 2, (16, 16, 16)  # the whole world, 4^3 voxels per cell
    o3, d3 = _i3(0, 0, 0), _i3(*dims)
    nw = dims[1] * dims[2]
    work = torch.zeros(int(L.vxrt_lod_workspace_bytes(d3, shift)), dtype=torch.uint8, device="cuda")
    d_bits, d_sum = _dev(torch, _sentinel(nw + 8)), _dev(torch, _sentinel(8))
    assert L.vxrt_downsample_region(h, o3, d3, shift, 1, work.data_ptr(), d_bits.data_ptr(), None, d_sum.data_ptr(), None) == 0
    torch.cuda.synchronize()
    bits, summ = _sentinel(nw + 8), _sentinel(8)
    assert L.vxrt_downsample_region_host(h, o3, d3, shift, 1, bits.ctypes.data, None, summ.ctypes.data) == 0
    assert np.array_equal(summ, _words(d_sum)) and np.array_equal(bits, _words(d_bits))
    assert (bits[nw:] == SENTINEL).all() and 0 < int(summ[2]) < dims[0] * dims[1] * dims[2]  # cells set: some, not all
