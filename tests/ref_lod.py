"""Restatements of the occupancy LOD (include/vxrt.h, vxrt_downsample_region) from its definition, never from the code
under test: the counts of a box of cells three ways -- a padded source box summed over a (X, f, Y, f, Z, f) reshape, 3-D
prefix sums differenced at the eight corners of a cell, and a loop over the voxels of every cell for tiny boxes -- and the
bits, the packed words and the summary that follow from the counts.  A world is a bool [x, y, z] numpy grid; voxels outside
it are empty."""
from typing import NamedTuple

import numpy as np

MAX_SHIFT = 5


def source_box(world, origin, dims, shift):
    """the f * dims voxels at `origin` as a bool [x, y, z] grid, empty outside the world"""
    f = 1 << shift
    S = [f * int(d) for d in dims]
    out = np.zeros(S, bool)
    lo = [max(int(o), 0) for o in origin]
    hi = [min(int(o) + s, n) for o, s, n in zip(origin, S, world.shape)]
    if all(a < b for a, b in zip(lo, hi)):
        dst = tuple(slice(a - int(o), b - int(o)) for a, b, o in zip(lo, hi, origin))
        out[dst] = world[tuple(slice(a, b) for a, b in zip(lo, hi))]
    return out


def counts_reshape(world, origin, dims, shift):
    f = 1 << shift
    X, Y, Z = (int(d) for d in dims)
    return source_box(world, origin, dims, shift).reshape(X, f, Y, f, Z, f).sum(axis=(1, 3, 5), dtype=np.int64)


def counts_prefix(world, origin, dims, shift):
    """P[i, j, k] = solid voxels of the world in [0, i) x [0, j) x [0, k); a cell's count is the signed sum of P at the eight
    corners of the cell clipped to the world"""
    f = 1 << shift
    P = np.zeros([n + 1 for n in world.shape], np.int64)
    P[1:, 1:, 1:] = world.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    edges = [np.clip(int(o) + f * np.arange(int(d) + 1, dtype=np.int64), 0, n) for o, d, n in zip(origin, dims, world.shape)]
    a, b, c = edges
    Q = P[np.ix_(a, b, c)]
    return (Q[1:, 1:, 1:] - Q[:-1, 1:, 1:] - Q[1:, :-1, 1:] - Q[1:, 1:, :-1] + Q[:-1, :-1, 1:] + Q[:-1, 1:, :-1] + Q[1:, :-1, :-1]
            - Q[:-1, :-1, :-1])


def counts_brute(world, origin, dims, shift):
    """voxel by voxel: tiny boxes only"""
    f = 1 << shift
    out = np.zeros([int(d) for d in dims], np.int64)
    for X in range(out.shape[0]):
        for Y in range(out.shape[1]):
            for Z in range(out.shape[2]):
                for x in range(int(origin[0]) + f * X, int(origin[0]) + f * X + f):
                    for y in range(int(origin[1]) + f * Y, int(origin[1]) + f * Y + f):
                        for z in range(int(origin[2]) + f * Z, int(origin[2]) + f * Z + f):
                            if 0 <= x < world.shape[0] and 0 <= y < world.shape[1] and 0 <= z < world.shape[2] and world[x, y, z]:
                                out[X, Y, Z] += 1
    return out


def pack(bits):
    """bool [x, y, z] -> region words: bit x & 31 of word x >> 5 of row (y, z), rows y fastest then z, padding bits 0"""
    X, Y, Z = bits.shape
    wpr = (X + 31) // 32
    words = np.zeros((Z, Y, wpr), np.uint32)
    for x in range(X):
        words[:, :, x >> 5] |= bits[x].T.astype(np.uint32) << np.uint32(x & 31)
    return words.reshape(-1)


def summary_words(counts, shift, threshold):
    """vxrt_lod_summary as eight uint32 words: solid (low, high), set, empty, full, mixed, max_count, reserved"""
    full = 1 << (3 * shift)
    solid = int(counts.sum())
    return np.array([solid & 0xFFFFFFFF, solid >> 32, int((counts >= threshold).sum()), int((counts == 0).sum()),
                     int((counts == full).sum()), int(((counts > 0) & (counts < full)).sum()), int(counts.max()), 0], np.uint32)


class Lod(NamedTuple):
    bits: np.ndarray      # bool [x, y, z]
    counts: np.ndarray    # uint16 [x, y, z]
    words: np.ndarray     # region words of the bits
    flat: np.ndarray      # the counts in region order (x fastest, then y, then z)
    summary: np.ndarray   # summary_words


def downsample(world, origin, dims, shift, threshold, counts=None):
    c = counts_prefix(world, origin, dims, shift) if counts is None else counts
    assert 1 <= shift <= MAX_SHIFT and 1 <= threshold <= 1 << (3 * shift) and c.max() <= 1 << (3 * shift)
    bits = c >= threshold
    return Lod(bits, c.astype(np.uint16), pack(bits), c.astype(np.uint16).transpose(2, 1, 0).reshape(-1),
               summary_words(c, shift, threshold))


def workspace_bytes(dims, shift):
    """the formula of include/vxrt.h"""
    if not 1 <= shift <= MAX_SHIFT or any(d < 1 for d in dims):
        return 0
    S = [int(d) << shift for d in dims]
    if S[0] * S[1] * S[2] > 1 << 32:
        return 0
    return -(-(4 * -(-S[0] // 32) * S[1] * S[2]) // 256) * 256


def fnv1a(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h
