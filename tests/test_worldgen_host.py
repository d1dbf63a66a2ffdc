"""tests/ref_worldgen.py (the numpy restatement of the column generators and of the tables that follow from heights) held
bit-equal to the oracle's builder, hand-derived cases of both, and vxo.gen_bricks (single cells straight from the
generator) against the same cells of a whole oracle world.  No GPU."""
import numpy as np
import pytest

from tests import ref_worldgen as rw

CDIMS = [(8, 16, 24), (24, 8, 16)]      # three different cell counts per axis, and a permutation
EMPTY = 0xFFFFFFFF


@pytest.mark.parametrize("cdims", CDIMS)
@pytest.mark.parametrize("f", [8, 16, 32])
@pytest.mark.parametrize("gen", [rw.GEN_HASH_HEIGHTFIELD, rw.GEN_INT_TERRAIN])
def test_numpy_restatement_equals_the_oracle_builder(vxo, gen, f, cdims):
    X, Y, Z = (c * f for c in cdims)
    w = vxo.World.generate(gen, X, Y, Z, f, nthreads=16)
    ref = rw.RefWorld(gen, X, Y, Z, f)
    t = ref.tables()
    assert t["nslots"] == w.nslots and 0 < w.nslots < w.ncells
    assert np.array_equal(t["coarse_bits"], w.coarse_bits)
    assert np.array_equal(t["brick_slot"], w.brick_slot)
    assert np.array_equal(t["bounds"].view(np.uint32), w.bounds.view(np.uint32))
    occ, slots, nslots = ref.occupancy_and_slots()
    assert nslots == w.nslots and np.array_equal(slots, w.brick_slot) and np.array_equal(occ, w.brick_slot != EMPTY)
    bw = f ** 3 // 32
    assert np.array_equal(ref.brick_images(np.flatnonzero(occ)), w.pool.reshape(-1, bw))
    assert not ref.brick_images(np.flatnonzero(~occ)[:64]).any()


def _oracle_heights(vxo, gen, X, Y, Z, top):
    L = vxo.lib()
    return np.array([[sum(L.vxo_gen_solid(gen, x, y, z, X, Y, Z) for y in range(top)) for z in range(Z)] for x in range(X)])


def test_degenerate_branches_of_the_height_functions(vxo):
    """HASH_HEIGHTFIELD with 3Y/8 == 0 (the range forced to 1) and with range 1: a flat base 3Y/16 = 0; the first Y with a
    range above 1; INT_TERRAIN with amplitude 0 from the first octave (Y = 1: height Y/8 = 0) and from a later one."""
    for Y in (1, 2, 3, 5):                                  # 3Y/8 = 0, 0, 1, 1: hash % 1 == 0, so h = 3Y/16 = 0
        assert not rw.hash_heights(24, Y, 40).any()
    h = rw.hash_heights(64, 8, 64)                          # base 1, range 3
    assert h.min() == 1 and h.max() == 3 and np.array_equal(h, _oracle_heights(vxo, rw.GEN_HASH_HEIGHTFIELD, 64, 8, 64, 8))
    assert np.array_equal(h[::8, ::8].repeat(8, 0).repeat(8, 1), h)      # constant on 8 x 8 footprints
    assert not rw.terrain_heights(40, 1, 24).any()          # amp = 0 at once, h = 1 / 8
    assert (rw.terrain_heights(40, 15, 24) >= 1).all()      # Y / 8 = 1
    for Y in (2, 8, 15):                                    # amplitudes (1), (4, 2, 1), (7, 3, 1): the loop ends early
        assert np.array_equal(rw.terrain_heights(300, Y, 70), _oracle_heights(vxo, rw.GEN_INT_TERRAIN, 300, Y, 70, 2 * Y + 2))
    # a lattice value hash % 1 is 0, so Y = 2 (amplitude 1 once) is flat as well
    assert not rw.terrain_heights(300, 2, 70).any()


def test_hash_words_against_the_oracle(vxo):
    s = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x12345678, 73856093, 4096], np.uint64)
    assert [int(v) for v in rw.g_hash32(s)] == [vxo.hash32(int(v)) for v in s]


def test_a_brick_cut_by_the_surface_by_hand(vxo):
    """Two columns in the brick column (bx, bz) = (1, 2) of a 64^3 world at f = 8: (x, z) = (10, 19) 13 voxels tall,
    (13, 22) 10 voxels tall.  Cell (1, 0, 2) holds both to its full height, cell (1, 1, 2) 5 and 2 voxels of them."""
    h = np.zeros((64, 64), np.int64)
    h[10, 19], h[13, 22] = 13, 10
    ref = rw.RefWorld(None, 64, 64, 64, 8, h=h)
    t = ref.tables()
    lower, upper = 1 + 0 * 8 + 2 * 64, 1 + 1 * 8 + 2 * 64        # tiled index inside the only tile
    assert t["nslots"] == 2
    assert np.flatnonzero(t["brick_slot"] != EMPTY).tolist() == [lower, upper]
    assert t["brick_slot"][lower] == 0 and t["brick_slot"][upper] == 1
    assert t["bounds"][lower].tolist() == [2, 0, 3, 5, 7, 6]
    assert t["bounds"][upper].tolist() == [2, 0, 3, 5, 4, 6]
    assert t["bounds"][0].tolist() == [0, 0, 0, -1, -1, -1]
    words = np.zeros(16, np.uint32)
    words[lower // 32] |= np.uint32(1 << (lower % 32))
    words[upper // 32] |= np.uint32(1 << (upper % 32))
    assert np.array_equal(t["coarse_bits"], words)
    img = ref.brick_images([lower, upper, 0])
    want = np.zeros((3, 16), np.uint32)
    for k, tall in ((0, (8, 8)), (1, (5, 2))):
        for (lx, lz), n in zip(((2, 3), (5, 6)), tall):
            for ly in range(n):
                bit = lx + ly * 8 + lz * 64
                want[k, bit // 32] |= np.uint32(1 << (bit % 32))
    assert np.array_equal(img, want)
    # and the oracle's builder on the same voxels
    vox = np.zeros((64, 64, 64), bool)
    vox[10, :13, 19] = vox[13, :10, 22] = True
    w = vxo.World.from_voxels(vox, 8)
    assert np.array_equal(t["coarse_bits"], w.coarse_bits) and np.array_equal(t["brick_slot"], w.brick_slot)
    assert np.array_equal(t["bounds"], w.bounds) and np.array_equal(img[:2].reshape(-1), w.pool)


@pytest.mark.parametrize("gen,shape,f", [(rw.GEN_HASH_HEIGHTFIELD, (64, 128, 64), 8), (rw.GEN_PERLIN_REF, (64, 64, 128), 8),
                                         (rw.GEN_INT_TERRAIN, (128, 128, 256), 16),
                                         (rw.GEN_HASH_HEIGHTFIELD, (256, 256, 256), 32)])
def test_gen_bricks_equals_the_cells_of_a_whole_world(vxo, gen, shape, f):
    w = vxo.World.generate(gen, *shape, f, nthreads=16)
    bw = f ** 3 // 32
    occ = w.brick_slot != EMPTY
    want = np.zeros((w.ncells, bw), np.uint32)
    want[occ] = w.pool.reshape(-1, bw)
    cells = np.arange(w.ncells)
    rng = np.random.default_rng(gen * 100 + f)
    pick = rng.integers(0, cells.size, 300)                  # shuffled, with repeats
    pick[10:20] = pick[0]
    for c in (cells, cells[pick]):
        g = vxo.gen_bricks(gen, *shape, f, c, nthreads=16)
        assert np.array_equal(g["any"], occ[c])
        assert np.array_equal(g["bounds"].view(np.uint32), w.bounds[c].view(np.uint32))
        assert np.array_equal(g["pool"], want[c])
    assert occ[cells].any() and not occ[cells].all()
    with pytest.raises(ValueError):
        vxo.gen_bricks(gen, *shape, f, [w.ncells])
    for wild in (np.array([1 << 32], np.int64), np.array([-1]), np.array([0.5])):   # would wrap to a cell in a cast
        with pytest.raises(ValueError):
            vxo.gen_bricks(gen, *shape, f, wild)
    with pytest.raises(ValueError):
        vxo.gen_bricks(gen, shape[0] + 8, shape[1], shape[2], f, [0])
    assert vxo.gen_bricks(gen, *shape, f, [])["pool"].shape == (0, bw)
