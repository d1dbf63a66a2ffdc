"""Two restatements of the chunk-streaming contract (include/vxrt.h, vxrt_stream_focus) on a world's tables:
  StreamModelA  the pool as a sorted list of free ranges [start, length], first fit over it, a released range merged with
                the ranges that end where it starts and start where it ends (as the header describes);
  StreamModelB  the pool as one flag per brick, the lowest run of n free bricks found by scanning the flags, so merging
                free ranges is implicit (an independent check of the library's release()).
Both take the chunk table from a world's coarse bits (Tables; Tables.of(world) for an oracle World) and return per call
{"rc", "stats" (the eight vxrt_stream_stats fields, None unless rc == OK), "flags", "base"}.  `src` holds, per cache
slot, the file slot whose brick it last received (-1: never written), from which expected_cache derives the tables and
the whole pool that vxrt_download_world returns, stale bricks included.  TEST INFRASTRUCTURE ONLY: imported by tests/
alone."""
from __future__ import annotations

import numpy as np

F32 = np.float32
EMPTY = 0xFFFFFFFF
OK, INVALID, READ_FAILED = "ok", "invalid", "read_failed"
STAT_FIELDS = ("chunks_total", "chunks_occupied", "chunks_resident", "bricks_resident", "chunks_loaded", "chunks_evicted",
               "chunks_missing", "bytes_read")


class Tables:
    """The chunk table of a world: a chunk is one 8x8x8 tile of coarse cells, cells ch * 512 .. ch * 512 + 511 of the
    tiled-linear tables; its bricks are one run of the file's slots, in cell order."""

    def __init__(self, factor, cdims, coarse_bits):
        self.factor = int(factor)
        self.cdims = tuple(int(c) for c in cdims)
        ncells = int(np.prod(self.cdims))
        self.nchunks = ncells // 512
        occ = np.unpackbits(np.asarray(coarse_bits, "<u4").view(np.uint8), bitorder="little")[:ncells].astype(bool)
        self.occupied = occ
        self.nbricks = occ.reshape(self.nchunks, 512).sum(axis=1).astype(np.int64)
        self.first_slot = np.concatenate([[0], np.cumsum(self.nbricks)[:-1]]).astype(np.int64)
        self.nslots = int(self.nbricks.sum())
        self.brick_bytes = self.factor ** 3 // 8
        tw, th = self.cdims[0] // 8, self.cdims[1] // 8
        ch = np.arange(self.nchunks)
        t = np.stack([ch % tw, (ch // tw) % th, ch // (tw * th)], axis=1)
        e = F32(8.0) * F32(self.factor)
        self.lo = t.astype(F32) * e                  # [8f t, 8f (t + 1)] per axis, binary32
        self.hi = self.lo + e

    @staticmethod
    def of(world):
        t = Tables(world.factor, world.cdims, world.coarse_bits)
        occ = world.brick_slot != EMPTY
        assert np.array_equal(occ, t.occupied), "cell table and coarse bits disagree"
        assert np.array_equal(world.brick_slot[occ], np.arange(t.nslots)), "slots are not in cell order"
        return t

    def d2(self, focus):
        """binary32 squared distance of `focus` to every chunk's box: per-axis gaps squared, summed in x, y, z order"""
        f = np.asarray(focus, F32)
        with np.errstate(over="ignore"):    # a far focus: d^2 = +inf, as in binary32
            d = np.where(f < self.lo, self.lo - f, np.where(f > self.hi, f - self.hi, F32(0.0))).astype(F32)
            sq = (d * d).astype(F32)
            return ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)


def focus_valid(focus, radius):
    f = np.asarray(focus, F32)
    return bool(np.isfinite(f).all()) and bool(F32(radius) >= F32(0.0))


class _Model:
    """The policy of vxrt_stream_focus; subclasses own the pool (_alloc, _release)."""

    def __init__(self, tables: Tables, capacity: int):
        assert 0 < capacity <= EMPTY
        self.t = tables
        self.capacity = int(capacity)
        self.base = np.full(tables.nchunks, -1, np.int64)
        self.src = np.full(self.capacity, -1, np.int64)
        self._init_pool()

    def flags(self):
        return (self.base >= 0).astype(np.uint8)

    def _result(self, rc, stats=None):
        return {"rc": rc, "stats": stats, "flags": self.flags(), "base": self.base.copy()}

    def focus(self, focus, radius, unreadable=()):
        """one call; `unreadable`: chunks whose read from the file fails"""
        if not focus_valid(focus, radius):
            return self._result(INVALID)
        t = self.t
        d2 = t.d2(focus)
        occupied = np.flatnonzero(t.nbricks > 0)
        order = occupied[np.argsort(d2[occupied], kind="stable")]     # ties: the lower chunk index first
        r2 = F32(F32(radius) * F32(radius))
        inside = [int(c) for c in order if d2[c] <= r2]
        candidates = iter([int(c) for c in order[::-1] if not d2[c] <= r2])  # eviction: farthest first, each seen once
        loaded = evicted = missing = nbytes = 0
        for ch in inside:
            if self.base[ch] >= 0:
                continue
            n = int(t.nbricks[ch])
            start = self._alloc(n)
            while start is None:
                v = next(candidates, None)
                if v is None:
                    break
                if self.base[v] < 0:
                    continue
                self._release(int(self.base[v]), int(t.nbricks[v]))
                self.base[v] = -1
                evicted += 1
                start = self._alloc(n)
            if start is None:
                missing += 1
                continue
            if ch in unreadable:
                self._release(start, n)
                return self._result(READ_FAILED)
            self.base[ch] = start
            self.src[start:start + n] = t.first_slot[ch] + np.arange(n)
            loaded += 1
            nbytes += n * t.brick_bytes
        res = self.base >= 0
        stats = (t.nchunks, int((t.nbricks > 0).sum()), int(res.sum()), int(t.nbricks[res].sum()), loaded, evicted, missing,
                 nbytes)
        return self._result(OK, stats)


class StreamModelA(_Model):
    """free ranges, first fit, merging on release"""

    def _init_pool(self):
        self.free = [[0, self.capacity]]

    def _alloc(self, n):
        for i, (s, ln) in enumerate(self.free):
            if ln >= n:
                if ln == n:
                    del self.free[i]
                else:
                    self.free[i] = [s + n, ln - n]
                return s
        return None

    def _release(self, start, n):
        i = 0
        while i < len(self.free) and self.free[i][0] < start:
            i += 1
        self.free.insert(i, [start, n])
        if i + 1 < len(self.free) and start + n == self.free[i + 1][0]:   # the range that starts where this one ends
            self.free[i][1] += self.free[i + 1][1]
            del self.free[i + 1]
        if i > 0 and self.free[i - 1][0] + self.free[i - 1][1] == start:  # the range that ends where this one starts
            self.free[i - 1][1] += self.free[i][1]
            del self.free[i]


class StreamModelB(_Model):
    """one flag per brick; the lowest run of n free bricks by scanning"""

    def _init_pool(self):
        self.used = np.zeros(self.capacity, bool)

    def _alloc(self, n):
        free = np.concatenate([[False], ~self.used, [False]]).astype(np.int8)
        edges = np.diff(free)
        starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
        fit = np.flatnonzero(ends - starts >= n)
        if fit.size == 0:
            return None
        s = int(starts[fit[0]])
        self.used[s:s + n] = True
        return s

    def _release(self, start, n):
        assert self.used[start:start + n].all()
        self.used[start:start + n] = False


def expected_cache(world, model: _Model):
    """what vxrt_download_world returns for the model's cache: coarse_bits, brick_slot, bounds [ncells, 6], pool"""
    t = model.t
    coarse = np.zeros_like(world.coarse_bits)
    slot = np.full(world.brick_slot.shape, EMPTY, np.uint32)
    bounds = np.tile(np.array([0, 0, 0, -1, -1, -1], np.float32), (world.brick_slot.size, 1))
    wb = np.asarray(world.bounds, np.float32).reshape(-1, 6)
    for ch in np.flatnonzero(model.base >= 0):
        coarse[ch * 16:(ch + 1) * 16] = world.coarse_bits[ch * 16:(ch + 1) * 16]
        cells = ch * 512 + np.flatnonzero(t.occupied[ch * 512:(ch + 1) * 512])
        slot[cells] = model.base[ch] + np.arange(cells.size)
        bounds[cells] = wb[cells]
    bw = world.factor ** 3 // 32
    pool = np.zeros((model.capacity, bw), np.uint32)
    written = model.src >= 0
    pool[written] = np.asarray(world.pool).reshape(-1, bw)[model.src[written]]
    return {"coarse_bits": coarse, "brick_slot": slot, "bounds": bounds, "pool": pool.reshape(-1)}


def truncated_world(vxo, world, flags):
    """the oracle world with the bricks of non-resident chunks removed (their cells unoccupied)"""
    coarse = world.coarse_bits.copy()
    slot = world.brick_slot.copy()
    for ch in np.flatnonzero(np.asarray(flags) == 0):
        coarse[ch * 16:(ch + 1) * 16] = 0
        slot[ch * 512:(ch + 1) * 512] = EMPTY
    return vxo.World.wrap(world.factor, world.cdims, coarse, slot, world.bounds, world.pool)
