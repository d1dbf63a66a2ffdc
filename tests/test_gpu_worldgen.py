"""The on-device world builder (vxrt_build_world_procedural) and the table transfers (upload, download, save, load) at the
sizes and shapes where their launches and copies change form:
  * every generator at every brick edge, on grids whose three cell counts differ, against the oracle's builder, or, where
    the oracle's whole world is out of reach (PERLIN_REF at f = 16 and 32), against single cells the oracle evaluates
    straight from the generator (vxo.gen_bricks) plus whole-table consistency
  * more cells than one row of the builder's 2-D launch grid holds (2^20), the last row ragged, against the numpy
    restatement of the column generators (tests/ref_worldgen.py)
  * a world whose cell table and pool both cross the 64 MiB pieces of save, load and download, unedited and edited
    (the compacting save)
  * worlds without a brick and with every voxel solid.
"""
import os

import numpy as np
import pytest

from tests import helpers
from tests import ref_worldgen as rw
from tests.helpers import eng, float_bits, new_ctx, upload   # noqa: F401  (eng is a fixture)

pytestmark = pytest.mark.gpu
EMPTY = 0xFFFFFFFF
HEADER_BYTES = 120


def _same_batch(a, b):
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["steps"], b["steps"])
    assert np.array_equal(a["voxel"], b["voxel"])
    assert np.array_equal(float_bits(a["hitPoint"]), float_bits(b["hitPoint"]))
    assert np.array_equal(float_bits(a["normal"]), float_bits(b["normal"]))


def _same_download(a, b):
    assert a["factor"] == b["factor"] and tuple(a["cdims"]) == tuple(b["cdims"])
    for k in ("coarse_bits", "brick_slot", "pool"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["bounds"].view(np.uint32), b["bounds"].view(np.uint32))


def sample_cells(cdims, n, seed):
    """n distinct tiled cell indices: the eight corner cells, the rest seeded"""
    cx, cy, cz = cdims
    corners = [rw.tiled_index(x, y, z, cx, cy) for x in (0, cx - 1) for y in (0, cy - 1) for z in (0, cz - 1)]
    order = np.random.default_rng(seed).permutation(cx * cy * cz)
    rest = order[~np.isin(order, corners)][:n - 8]          # the first n - 8 of the seeded order that are no corner
    return np.concatenate([np.asarray(corners, np.int64), rest])


# ---- a. every generator at every brick edge ---------------------------------------------------------------------------
@pytest.mark.parametrize("cdims", [(8, 16, 24), (24, 8, 16)])
@pytest.mark.parametrize("f", [8, 16, 32])
@pytest.mark.parametrize("gen", [rw.GEN_HASH_HEIGHTFIELD, rw.GEN_PERLIN_REF, rw.GEN_INT_TERRAIN])
def test_every_generator_at_every_brick_edge(eng, vxo, gen, f, cdims):
    vx, _ = eng
    X, Y, Z = (c * f for c in cdims)
    ctx = new_ctx(vx)
    try:
        info = ctx.build_world(gen, X, Y, Z, f)
        d = ctx.download_world()
    finally:
        ctx.close()
    assert tuple(info.cdims) == cdims and info.factor == f and info.ncells == cdims[0] * cdims[1] * cdims[2]
    rw.assert_consistent(d, int(info.nslots))
    if gen != rw.GEN_PERLIN_REF or f == 8:
        w = vxo.World.generate(gen, X, Y, Z, f, nthreads=16)
        assert info.nslots == w.nslots
        assert np.array_equal(d["coarse_bits"], w.coarse_bits)
        assert np.array_equal(d["brick_slot"], w.brick_slot)
        assert np.array_equal(d["bounds"].view(np.uint32), w.bounds.view(np.uint32))
        assert np.array_equal(d["pool"], w.pool)
        return
    # PERLIN_REF at f = 16, 32: 128 cells straight from the oracle's generator.  The oracle alone decides the three kinds.
    cells = sample_cells(cdims, 128, seed=f)
    assert cells.size == 128 and np.unique(cells).size == 128
    cx, cy, cz = cdims
    for corner in [(x, y, z) for x in (0, cx - 1) for y in (0, cy - 1) for z in (0, cz - 1)]:
        assert rw.tiled_index(*corner, cx, cy) in cells[:8]
    g = vxo.gen_bricks(gen, X, Y, Z, f, cells, nthreads=16)
    rw.assert_cells_match_generator(d, cells, g)


# ---- b. two rows of the builder's launch grid, the second ragged ------------------------------------------------------
@pytest.mark.parametrize("gen", [rw.GEN_INT_TERRAIN, rw.GEN_HASH_HEIGHTFIELD])
def test_more_cells_than_one_grid_row(eng, gen):
    """1088 x 512 x 1024 at f = 8: 136 x 64 x 128 = 2^20 + 65 536 cells, so k_fill_bricks and k_pack_bricks run a
    (2^20, 2) grid whose second row is mostly past the last cell."""
    vx, _ = eng
    X, Y, Z, f = 1088, 512, 1024, 8
    bw = f ** 3 // 32
    ref = rw.RefWorld(gen, X, Y, Z, f)
    t = ref.tables()
    assert ref.ncells == (1 << 20) + 65536
    if gen == rw.GEN_INT_TERRAIN:
        assert t["nslots"] == 706715
    ctx, twin = new_ctx(vx), new_ctx(vx)
    try:
        info = ctx.build_world(gen, X, Y, Z, f)
        d = ctx.download_world()
        assert info.nslots == t["nslots"] and info.ncells == ref.ncells
        assert np.array_equal(d["coarse_bits"], t["coarse_bits"])
        assert np.array_equal(d["brick_slot"], t["brick_slot"])
        assert np.array_equal(d["bounds"].view(np.uint32), t["bounds"].view(np.uint32))
        assert d["pool"].size == t["nslots"] * bw
        # brick bits: slot 0, the last slot, the occupied cells on both sides of the tiled indices 2^20 - 1, 2^20 and
        # ncells - 1, and a seeded 50 000 more
        cells_of_slot = np.flatnonzero(t["brick_slot"] != EMPTY)
        must = [0, t["nslots"] - 1]
        for at in ((1 << 20) - 1, 1 << 20, ref.ncells - 1):
            k = int(np.searchsorted(cells_of_slot, at))
            must += [min(max(k + j, 0), t["nslots"] - 1) for j in (-1, 0, 1)]
        assert cells_of_slot[must].max() >= 1 << 20 and cells_of_slot[must].min() < 1 << 20
        rng = np.random.default_rng(gen)
        slots = np.unique(np.concatenate([np.asarray(must, np.int64), rng.permutation(t["nslots"])[:50000]]))
        assert np.array_equal(d["pool"].reshape(-1, bw)[slots], ref.brick_images(cells_of_slot[slots]))
        # upload against build: the downloaded tables, uploaded into a second context, trace alike bit for bit
        twin.upload_world(f, d["cdims"], d["coarse_bits"], d["brick_slot"], d["bounds"], d["pool"])
        o, dr = helpers.mixed_rays((X, Y, Z), 20000, seed=gen)
        a, b = ctx.Raytrace(o, dr), twin.Raytrace(o, dr)
        assert 0 < int(a["hit"].sum()) < 20000
        _same_batch(a, b)
    finally:
        ctx.close()
        twin.close()


# ---- d. transfers in several 64 MiB pieces ------------------------------------------------------------------------------
def test_transfers_in_several_pieces(eng, tmp_path):
    """2112 x 512 x 4096 INT_TERRAIN at f = 8: 264 x 64 x 512 = 8 650 752 cells (a 69.2 MB cell table: a 64 MiB piece and
    one of 2 MiB) and 5 113 832 bricks (a 327 MB pool: four 64 MiB pieces and a ragged fifth); the builder's grid has 9
    rows, the last one ragged."""
    vx, _ = eng
    X, Y, Z, f = 2112, 512, 4096, 8
    cd = (X // f, Y // f, Z // f)
    bw = f ** 3 // 32
    ncells = cd[0] * cd[1] * cd[2]
    ref = rw.RefWorld(rw.GEN_INT_TERRAIN, X, Y, Z, f)
    occ, slots, nslots = ref.occupancy_and_slots()
    assert ncells == 8650752 and nslots == 5113832
    assert ncells * 8 > 64 << 20 and nslots * bw * 4 > 4 * (64 << 20)
    table_bytes = ncells // 8 + ncells * 8
    path, path2 = str(tmp_path / "big.vxb"), str(tmp_path / "edited.vxb")
    ctx, other = new_ctx(vx), new_ctx(vx)
    try:
        # 1, 2: build, download
        info = ctx.build_world(rw.GEN_INT_TERRAIN, X, Y, Z, f)
        d0 = ctx.download_world()
        assert info.nslots == nslots and info.ncells == ncells
        assert np.array_equal(d0["brick_slot"], slots)
        rw.assert_consistent(d0, nslots)
        # 3: save
        ctx.save_world(path)
        fi = vx.world_file_info(path)
        assert (fi.factor, tuple(fi.cdims), fi.ncells, fi.nslots) == (f, cd, ncells, nslots)
        assert fi.hbm_bytes == info.hbm_bytes == table_bytes + nslots * bw * 4
        assert os.path.getsize(path) == HEADER_BYTES + fi.hbm_bytes
        # 4: load into a second context
        got = other.load_world(path)
        assert got.nslots == nslots
        _same_download(other.download_world(), d0)
        os.remove(path)
        # 5: upload the download into a third context
        third = new_ctx(vx)
        try:
            third.upload_world(f, d0["cdims"], d0["coarse_bits"], d0["brick_slot"], d0["bounds"], d0["pool"])
            _same_download(third.download_world(), d0)
        finally:
            third.close()
        del d0
        # 6: edits.  A box of sky set first: its bricks are appended behind the last piece of the pool; then a brick-aligned
        # slab cleared half way along z: its bricks go from the middle pieces, and every later brick of the file moves up.
        sky = (8, 59, 8), (23, 60, 9)                     # cells (lo, hi inclusive), above the tallest column
        slab_z = 256
        cells = np.arange(ncells, dtype=np.int64)
        bx, by, bz = rw.tiled_cell(cells, cd[0], cd[1])
        in_sky = ((bx >= sky[0][0]) & (bx <= sky[1][0]) & (by >= sky[0][1]) & (by <= sky[1][1]) & (bz >= sky[0][2]) & (bz <= sky[1][2]))
        in_slab = bz == slab_z
        del bx, by, bz, cells
        assert not occ[in_sky].any() and int(in_sky.sum()) == 16 * 2 * 2
        freed = int(occ[in_slab].sum())
        first_freed = int(slots[in_slab & occ].min())
        assert freed > 5000 and (64 << 20) // (bw * 4) < first_freed < nslots - (64 << 20) // (bw * 4)
        st = ctx.edit_voxels([vx.EditBox([c * f for c in sky[0]], [c * f + f - 1 for c in sky[1]], 1)])
        assert st.bricks_created == 64 and st.bricks_freed == 0 and st.pool_slots == nslots + 64
        st = ctx.edit_voxels([vx.EditBox((0, 0, slab_z * f), (X - 1, Y - 1, slab_z * f + f - 1), 0)])
        assert st.bricks_freed == freed and st.bricks_created == 0
        live = nslots + 64 - freed
        assert st.bricks_live == live and st.pool_slots == nslots + 64
        want_occ = (occ | in_sky) & ~in_slab
        del occ, slots, in_sky, in_slab
        e = ctx.download_world()
        e_occ = e["brick_slot"] != EMPTY
        assert np.array_equal(e_occ, want_occ)
        del want_occ
        # 7: the compacting save; 8: load and download
        ctx.save_world(path2)
        fi = vx.world_file_info(path2)
        assert fi.nslots == live and os.path.getsize(path2) == HEADER_BYTES + table_bytes + live * bw * 4
        got = other.load_world(path2)
        os.remove(path2)
        assert got.nslots == live
        ld = other.download_world()
        assert np.array_equal(ld["coarse_bits"], e["coarse_bits"])
        assert np.array_equal(ld["bounds"].view(np.uint32), e["bounds"].view(np.uint32))
        assert np.array_equal(ld["brick_slot"] != EMPTY, e_occ)
        assert np.array_equal(ld["brick_slot"][e_occ], np.arange(live, dtype=np.uint32))   # renumbered in tiled order
        e_slots = e["brick_slot"][e_occ]
        seen = np.zeros(e["pool"].size // bw, bool)
        seen[e_slots] = True
        assert int(seen.sum()) == live                                                   # no slot shared by two cells
        lp, ep = ld["pool"].reshape(-1, bw), e["pool"].reshape(-1, bw)
        assert lp.shape[0] == live
        for at in range(0, live, 1 << 20):                                               # brick bits through the slots
            assert np.array_equal(lp[at:at + (1 << 20)], ep[e_slots[at:at + (1 << 20)]]), at
    finally:
        ctx.close()
        other.close()
        for p in (path, path2):
            if os.path.exists(p):
                os.remove(p)


# ---- e. degenerate worlds ---------------------------------------------------------------------------------------------
def _round_trip(vx, ctx, w, path):
    """upload, download, save, world_file_info, load into another context, download: the oracle world's tables each time"""
    bw = w.factor ** 3 // 32
    upload(ctx, w)
    info = ctx.world_info()
    assert info.nslots == w.nslots and info.hbm_bytes == w.ncells // 8 + w.ncells * 8 + w.nslots * bw * 4
    want = dict(factor=w.factor, cdims=w.cdims, coarse_bits=w.coarse_bits, brick_slot=w.brick_slot, bounds=w.bounds, pool=w.pool)
    _same_download(ctx.download_world(), want)
    ctx.save_world(path)
    fi = vx.world_file_info(path)
    assert (fi.factor, tuple(fi.cdims), fi.ncells, fi.nslots, fi.hbm_bytes) == (w.factor, w.cdims, w.ncells, w.nslots, info.hbm_bytes)
    assert os.path.getsize(path) == HEADER_BYTES + fi.hbm_bytes
    other = new_ctx(vx)
    try:
        assert other.load_world(path).nslots == w.nslots
        _same_download(other.download_world(), want)
        return other
    except BaseException:
        other.close()
        raise


def _rays_and_frame(vx, torch, vxo, ctx, w):
    o, d = helpers.mixed_rays(w.dims, 20000, seed=w.factor)
    g, c = ctx.Raytrace(o, d), w.trace_batch(o, d, nthreads=16)
    assert np.array_equal(g["hit"], c["hit"]) and np.array_equal(g["steps"], c["steps"]) and np.array_equal(g["voxel"], c["voxel"])
    assert np.array_equal(float_bits(g["hitPoint"]), float_bits(c["pos"]))
    assert np.array_equal(float_bits(g["normal"]), float_bits(c["normal"]))
    got = helpers.render_frame(vx, ctx, torch, "A", w.dims, vxo, vx.MODE_SHADED)
    assert np.array_equal(got, helpers.oracle_frame(vxo, w, "A", w.dims, vx.MODE_SHADED))
    return g


@pytest.mark.parametrize("f", [8, 16, 32])
def test_a_world_without_a_brick(eng, vxo, tmp_path, f):
    vx, torch = eng
    n = 8 * f
    w = vxo.World.from_voxels(np.zeros((n, n, n), bool), f)
    assert w.nslots == 0 and w.pool.size == 0 and not w.coarse_bits.any() and (w.brick_slot == EMPTY).all()
    ctx = new_ctx(vx)
    others = []
    try:
        others.append(_round_trip(vx, ctx, w, str(tmp_path / "empty.vxb")))
        for c in (ctx, others[0]):               # the uploaded and the loaded world
            assert not _rays_and_frame(vx, torch, vxo, c, w)["hit"].any()
        # the same world reached through edits: a built world cleared by one box over all of it
        built = ctx.build_world(vx.GEN_INT_TERRAIN, n, n, n, f)
        st = ctx.edit_voxels([vx.EditBox((0, 0, 0), (n - 1, n - 1, n - 1), 0)])
        assert built.nslots > 0 and st.bricks_freed == built.nslots and st.bricks_live == 0
        path = str(tmp_path / "cleared.vxb")
        ctx.save_world(path)
        fi = vx.world_file_info(path)
        assert fi.nslots == 0 and os.path.getsize(path) == HEADER_BYTES + w.ncells // 8 + w.ncells * 8
        others.append(new_ctx(vx))
        assert others[1].load_world(path).nslots == 0
        ld = others[1].download_world()
        assert ld["pool"].size == 0 and np.array_equal(ld["coarse_bits"], w.coarse_bits)
        assert np.array_equal(ld["brick_slot"], w.brick_slot) and np.array_equal(ld["bounds"], w.bounds)
        assert not _rays_and_frame(vx, torch, vxo, others[1], w)["hit"].any()
    finally:
        ctx.close()
        for c in others:
            c.close()


@pytest.mark.parametrize("f", [8, 16, 32])
def test_a_world_with_every_voxel_solid(eng, vxo, tmp_path, f):
    vx, torch = eng
    n = 8 * f
    w = vxo.World.from_voxels(np.ones((n, n, n), bool), f)
    assert w.nslots == 512 and (w.pool == 0xFFFFFFFF).all() and (w.coarse_bits == 0xFFFFFFFF).all()
    assert np.array_equal(w.brick_slot, np.arange(512, dtype=np.uint32))
    assert (w.bounds[:, :3] == 0).all() and (w.bounds[:, 3:] == f - 1).all()
    ctx = new_ctx(vx)
    other = None
    try:
        other = _round_trip(vx, ctx, w, str(tmp_path / "solid.vxb"))
        for c in (ctx, other):
            assert _rays_and_frame(vx, torch, vxo, c, w)["hit"].any()
    finally:
        ctx.close()
        if other is not None:
            other.close()
