"""The Python-only side of the query results (voxelengine_amd/engine.py) without a GPU: each lazy result class in its host
form (numpy summary words, no stream) decodes the words of include/vxrt.h into its NamedTuple, hands back the grids it was
given, and ExtractedSurface.decode unpacks the quad record's bit fields.  Box of 33 x 3 x 2: 33 crosses a word boundary in
x, and three different extents catch a wrong transpose."""

import numpy as np
import pytest

import voxelengine_amd as vx

DIMS = (33, 3, 2)
ORIGIN = (5, -6, 7)


def _words(n):
    """n distinct summary words, none of them small enough to be taken for another's index"""
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(0x9E3779B9)) | np.uint32(0x80000000)


def _grid(dtype):
    return (np.arange(33 * 3 * 2) * 2551 % 65521).astype(dtype).reshape(DIMS[::-1]).transpose(2, 1, 0)


def test_distance_summary_and_grid():
    w = _words(6)
    assert int(w[5]) != 0  # a non-zero high half of the sum
    g = _grid(np.uint16)
    d = vx.DistanceField(origin=ORIGIN, dims=DIMS, radius=9, mode=vx.DIST_TO_SOLID, dist2=g, _summary=w, _stream=None)
    s = d.summary
    assert isinstance(s, vx.DistanceSummary)
    assert (s.zero, s.near, s.far, s.max_d2) == tuple(int(x) for x in w[:4])
    assert s.sum_d2 == int(w[4]) | int(w[5]) << 32
    assert d.grid() is g and d.grid().shape == DIMS
    assert d.summary == s  # read twice


def test_lod_summary_and_grids():
    w = _words(8)
    bits = np.random.default_rng(1).random(DIMS) < 0.5
    counts = _grid(np.uint16)
    d = vx.Downsampled(origin=ORIGIN, dims=DIMS, shift=2, threshold=3, bits=bits, counts=counts, _summary=w, _stream=None)
    s = d.summary
    assert isinstance(s, vx.LodSummary)
    assert s.solid == int(w[0]) | int(w[1]) << 32 and int(w[1]) != 0
    assert (s.set, s.empty, s.full, s.mixed, s.max_count) == tuple(int(x) for x in w[2:7])
    assert d.grid() is bits and d.count_grid() is counts
    none = vx.Downsampled(origin=ORIGIN, dims=DIMS, shift=2, threshold=3, bits=bits, counts=None, _summary=w, _stream=None)
    with pytest.raises(ValueError):
        none.count_grid()


def test_light_summary_and_grid():
    w = _words(42)
    levels = _grid(np.uint8)
    f = vx.LightField(origin=ORIGIN, dims=DIMS, channels=vx.LIGHT_SKY | vx.LIGHT_BLOCK, levels=levels, _summary=w, _stream=None)
    s = f.summary
    v = [int(x) for x in w]
    assert isinstance(s, vx.LightSummary)
    assert (s.solid, s.exposed) == (v[0], v[1])
    assert s.hist_sky == tuple(v[2:18]) and s.hist_block == tuple(v[18:34])
    assert s.sum_sky == v[34] | v[35] << 32 and s.sum_block == v[36] | v[37] << 32
    assert (s.emitters_used, s.emitters_solid, s.emitters_far, s.emitters_invalid) == tuple(v[38:42])
    assert f.grid() is levels
    assert np.array_equal(f.sky(), levels >> 4) and np.array_equal(f.block(), levels & 15)


def test_surface_summary_and_decode():
    w = _words(16)
    w[3] = 2  # two quads written
    # vxrt_quad: pos = x | y << 10 | z << 20, ext = (w - 1) | (h - 1) << 10 | d << 20
    want = [(5, 32, 2, 1, 1, 3), (0, 1023, 0, 1000, 1024, 1)]  # (d, x, y, z, w, h)
    quads = np.asarray([[x | y << 10 | z << 20, (qw - 1) | (qh - 1) << 10 | d << 20] for d, x, y, z, qw, qh in want], np.uint32)
    e = vx.ExtractedSurface(origin=ORIGIN, dims=DIMS, mode=vx.SURF_CAP, quads=quads, vertices=None, triangles=None, _summary=w,
                            _stream=None)
    s = e.summary
    v = [int(x) for x in w]
    assert isinstance(s, vx.SurfaceSummary)
    assert (s.solid, s.faces, s.quads, s.written) == (v[0], v[1], v[2], 2)
    assert s.faces_dir == tuple(v[4:10]) and s.quads_dir == tuple(v[10:16])
    got = e.decode()
    assert len(got) == 6
    assert [tuple(int(col[i]) for col in got) for i in range(2)] == want
    # only the written records are decoded
    more = vx.ExtractedSurface(origin=ORIGIN, dims=DIMS, mode=vx.SURF_CAP, quads=np.concatenate([quads, quads]), vertices=None,
                               triangles=None, _summary=w, _stream=None)
    assert [len(col) for col in more.decode()] == [2] * 6


def test_voxelize_summary_and_grid():
    w = _words(8)
    bits = np.random.default_rng(2).random(DIMS) < 0.5
    m = vx.VoxelizedMesh(dims=DIMS, modes=vx.VOX_SURFACE, bits=bits, _summary=w, _stream=None)
    s = m.summary
    assert isinstance(s, vx.VoxelizeSummary)
    assert tuple(s) == tuple(int(x) for x in w[:7])  # the eighth word is reserved
    assert (s.set, s.surface, s.solid, s.triangles, s.invalid, s.degenerate, s.outside) == tuple(s)
    assert m.grid() is bits


def test_region_round_trip():
    v = np.random.default_rng(3).random(DIMS) < 0.5
    w = vx.pack_region(v)
    assert w.dtype == np.uint32 and w.size == vx.region_words(DIMS) == 2 * 3 * 2
    got = vx.unpack_region(w, DIMS)
    assert got.dtype == bool and got.shape == DIMS and np.array_equal(got, v)
