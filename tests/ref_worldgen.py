"""A second restatement of the column generators (HASH_HEIGHTFIELD, INT_TERRAIN of oracle/vxo_world.c and
voxelengine_amd/csrc/vxrt_worldgen.hip) and of the brickmap tables that follow from them, in vectorised numpy.

A voxel of a column generator is solid iff y < h(x, z), so everything the builders produce is a function of the heights:
a brick cell (bx, by, bz) holds the voxels of its f x f columns below their heights.  All integer arithmetic is uint64
with explicit 32-bit masks where the C code wraps.  Tables come out as the C ABI carries them: cells in the reference's
tiled order (8x8x8 tiles, x fastest inside and between tiles), brick bits in the same order inside a brick.
"""
import numpy as np

GEN_HASH_HEIGHTFIELD, GEN_PERLIN_REF, GEN_INT_TERRAIN = 0, 1, 2   # PERLIN_REF: a 3-D field, not restated here
EMPTY_SLOT = 0xFFFFFFFF
U = np.uint64
M32 = U(0xFFFFFFFF)


def g_hash32(s):
    """cudaNoise::hash on uint64 arrays holding 32-bit values"""
    s = np.asarray(s, U) & M32
    s = ((s + U(0x7ed55d16)) + (s << U(12))) & M32
    s = (s ^ U(0xc761c23c)) ^ (s >> U(19))
    s = ((s + U(0x165667b1)) + (s << U(5))) & M32
    s = ((s + U(0xd3a2646c)) & M32) ^ ((s << U(9)) & M32)
    s = ((s + U(0xfd7046c5)) + (s << U(3))) & M32
    s = (s ^ U(0xb55a4f09)) ^ (s >> U(16))
    return s


def g_hash2(a, b, seed):
    a, b = np.asarray(a, U) & M32, np.asarray(b, U) & M32
    return g_hash32(((a * U(73856093)) & M32) ^ ((b * U(19349663)) & M32) ^ U(seed))


def hash_heights(X, Y, Z):
    """h[x, z] of HASH_HEIGHTFIELD: 3Y/16 + hash2(x >> 3, z >> 3, 1) % (3Y/8), the range 1 where 3Y/8 is 0"""
    base, rng = U(3 * Y // 16), U(3 * Y // 8)
    if rng == 0:
        rng = U(1)
    x, z = np.arange(X, dtype=U)[:, None], np.arange(Z, dtype=U)[None, :]
    return base + g_hash2(x >> U(3), z >> U(3), 1) % rng


def terrain_heights(X, Y, Z):
    """h[x, z] of INT_TERRAIN: Y/8 plus four octaves (pitch 256, 128, 64, 32; amplitude (Y/2) >> o, the loop ending at the
    first amplitude 0) of bilinearly interpolated lattice values hash2(cx, cz, 7 + o) % amplitude"""
    x, z = np.arange(X, dtype=U), np.arange(Z, dtype=U)
    h = np.full((X, Z), Y // 8, U)
    for o in range(4):
        k = U(8 - o)
        S = U(1) << k
        amp = U((Y // 2) >> o)
        if amp == 0:
            break
        cx, cz = x >> k, z >> k
        fx, fz = (x & (S - U(1)))[:, None], (z & (S - U(1)))[None, :]
        lx, lz = np.arange(int(cx.max()) + 2, dtype=U), np.arange(int(cz.max()) + 2, dtype=U)
        v = g_hash2(lx[:, None], lz[None, :], 7 + o) % amp          # the lattice, one row and column past the world
        ix, iz = cx.astype(np.int64), cz.astype(np.int64)
        v00, v10 = v[np.ix_(ix, iz)], v[np.ix_(ix + 1, iz)]
        v01, v11 = v[np.ix_(ix, iz + 1)], v[np.ix_(ix + 1, iz + 1)]
        top = v00 * (S - fx) + v10 * fx
        bot = v01 * (S - fx) + v11 * fx
        h += (top * (S - fz) + bot * fz) >> (U(2) * k)
    return h


def heights(gen, X, Y, Z):
    if gen == GEN_HASH_HEIGHTFIELD:
        return hash_heights(X, Y, Z)
    if gen == GEN_INT_TERRAIN:
        return terrain_heights(X, Y, Z)
    raise ValueError("not a column generator")


def tiled_order(a):
    """a[x, y, z, ...] over a grid whose dimensions are multiples of 8 -> its entries in the reference's tiled order"""
    nx, ny, nz = a.shape[:3]
    rest = a.shape[3:]
    a = a.reshape(nx // 8, 8, ny // 8, 8, nz // 8, 8, *rest)
    return a.transpose(4, 2, 0, 5, 3, 1, *range(6, 6 + len(rest))).reshape(-1, *rest)


def tiled_index(x, y, z, nx, ny):
    """GetSampleIndex: the tiled index of (x, y, z) in a grid nx wide and ny high"""
    x, y, z = (np.asarray(v, np.int64) for v in (x, y, z))
    tile = x // 8 + (y // 8) * (nx // 8) + (z // 8) * (nx // 8) * (ny // 8)
    return tile * 512 + x % 8 + (y % 8) * 8 + (z % 8) * 64


def tiled_cell(i, nx, ny):
    """GetPositionFromSampleIndex: the inverse of tiled_index"""
    i = np.asarray(i, np.int64)
    tile, inside = i // 512, i % 512
    tw, th = nx // 8, ny // 8
    return ((tile % tw) * 8 + inside % 8, ((tile // tw) % th) * 8 + (inside // 8) % 8, (tile // (tw * th)) * 8 + inside // 64)


class RefWorld:
    """The tables of the world a column generator (or any height map ``h[x, z]``) builds at brick edge ``f``."""

    def __init__(self, gen, X, Y, Z, f, h=None):
        assert X % (8 * f) == 0 and Y % (8 * f) == 0 and Z % (8 * f) == 0
        self.dims, self.factor = (X, Y, Z), f
        self.cdims = (X // f, Y // f, Z // f)
        self.ncells = self.cdims[0] * self.cdims[1] * self.cdims[2]
        self.h = (heights(gen, X, Y, Z) if h is None else np.asarray(h)).astype(np.int64)
        assert self.h.shape == (X, Z)

    # ---- from the per-brick maximum height alone
    def occupancy_and_slots(self):
        """(occupied, slots, nslots) in tiled cell order: a cell is occupied iff its tallest column passes its floor"""
        cx, cy, cz = self.cdims
        f = self.factor
        hmax = self.h.reshape(cx, f, cz, f).max(axis=(1, 3))
        occ = tiled_order(hmax[:, None, :] > (np.arange(cy, dtype=np.int64) * f)[None, :, None])
        return (occ,) + self._slots(occ)

    @staticmethod
    def _slots(occ):
        run = np.cumsum(occ, dtype=np.int64)
        slots = np.where(occ, run - 1, EMPTY_SLOT).astype(np.uint32)
        return slots, int(run[-1])

    # ---- the full cell tables
    def tables(self):
        """dict(coarse_bits, brick_slot, bounds, nslots) as vxo.World holds them"""
        cx, cy, cz = self.cdims
        f = self.factor
        lo = np.zeros((cx, cy, cz, 3), np.float32)
        hi = np.full((cx, cy, cz, 3), -1, np.float32)
        occ = np.zeros((cx, cy, cz), bool)
        hb = self.h.reshape(cx, f, cz, f)
        hmax = hb.max(axis=(1, 3))
        for by in range(cy):
            y0 = by * f
            solid = hb > y0                                   # columns that reach into this layer of cells
            colx, colz = solid.any(axis=3), solid.any(axis=1)  # [cx, f, cz], [cx, cz, f]
            o = hmax > y0
            occ[:, by, :] = o
            lo[:, by, :, 0] = np.where(o, colx.argmax(axis=1), 0)
            hi[:, by, :, 0] = np.where(o, f - 1 - colx[:, ::-1, :].argmax(axis=1), -1)
            lo[:, by, :, 2] = np.where(o, colz.argmax(axis=2), 0)
            hi[:, by, :, 2] = np.where(o, f - 1 - colz[:, :, ::-1].argmax(axis=2), -1)
            hi[:, by, :, 1] = np.where(o, np.minimum(hmax - y0, f) - 1, -1)   # a solid column starts at the cell's floor
        occ_t = tiled_order(occ)
        slots, nslots = self._slots(occ_t)
        coarse = np.packbits(occ_t.astype(np.uint8), bitorder="little").view(np.uint32).copy()
        bounds = np.concatenate([tiled_order(lo), tiled_order(hi)], axis=1)
        return dict(coarse_bits=coarse, brick_slot=slots, bounds=bounds, nslots=nslots)

    # ---- brick bits
    def brick_images(self, cells, block=1 << 24):
        """(n, f^3/32) uint32: the bit images of the tiled cells ``cells``, in the in-brick tiled order (all zero for an
        empty cell); evaluated ``block`` voxels at a time"""
        cells = np.asarray(cells, np.int64).reshape(-1)
        f = self.factor
        out = np.empty((cells.size, f ** 3 // 32), np.uint32)
        step = max(1, block // f ** 3)
        l = np.arange(f, dtype=np.int64)
        for at in range(0, cells.size, step):
            bx, by, bz = tiled_cell(cells[at:at + step], self.cdims[0], self.cdims[1])
            hh = self.h[(bx * f)[:, None, None] + l[None, :, None], (bz * f)[:, None, None] + l[None, None, :]]   # [n, x, z]
            bits = ((by * f)[:, None, None, None] + l[None, None, :, None]) < hh[:, :, None, :]                    # [n, x, y, z]
            n = bits.shape[0]
            bits = bits.reshape(n, f // 8, 8, f // 8, 8, f // 8, 8).transpose(0, 5, 3, 1, 6, 4, 2).reshape(n, -1)
            out[at:at + n] = np.packbits(bits.astype(np.uint8), axis=1, bitorder="little").view(np.uint32)
        return out


def assert_consistent(d, nslots, block=1 << 16):
    """What every built world's download satisfies whatever its generator: coarse bit <=> slot not empty <=> the slot's
    brick has a bit set, the slots 0 .. nslots-1 in tiled cell order, the pool exactly nslots bricks (checked ``block``
    bricks at a time)."""
    slot = d["brick_slot"]
    bw = d["factor"] ** 3 // 32
    occ = slot != EMPTY_SLOT
    bits = np.unpackbits(d["coarse_bits"].view(np.uint8), bitorder="little")[:slot.size].astype(bool)
    assert np.array_equal(bits, occ)
    assert int(occ.sum()) == nslots and d["pool"].size == nslots * bw
    assert np.array_equal(slot[occ], np.arange(nslots, dtype=np.uint32))
    pool = d["pool"].reshape(-1, bw)
    for at in range(0, nslots, block):
        assert pool[at:at + block].any(axis=1).all(), at
    empty = d["bounds"][~occ]
    assert (empty[:, :3] == 0).all() and (empty[:, 3:] == -1).all()


def assert_cells_match_generator(d, cells, g):
    """The tiled cells ``cells`` of the download ``d`` against ``g`` = vxo.gen_bricks of the same cells: occupancy by slot
    and by coarse bit, bounds, and the brick bits through the slots.  ``g`` (the oracle alone) must hold all three kinds
    of cell: empty, solid throughout, and cut by the surface."""
    cells = np.asarray(cells, np.int64)
    bw = d["factor"] ** 3 // 32
    full = (g["pool"] == 0xFFFFFFFF).all(axis=1)
    assert (~g["any"]).any() and full.any() and (g["any"] & ~full).any()
    slot = d["brick_slot"][cells]
    assert np.array_equal(slot != EMPTY_SLOT, g["any"])
    bits = (d["coarse_bits"][cells >> 5] >> (cells & 31).astype(np.uint32)) & 1
    assert np.array_equal(bits.astype(bool), g["any"])
    assert np.array_equal(d["bounds"][cells].view(np.uint32), g["bounds"].view(np.uint32))
    got = np.zeros_like(g["pool"])
    got[g["any"]] = d["pool"].reshape(-1, bw)[slot[g["any"]]]
    assert np.array_equal(got, g["pool"])
