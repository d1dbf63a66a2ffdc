"""CPU checks of the box collision queries (include/vxrt.h, vxrt_move_boxes / vxrt_overlap_boxes): the two restatements of
tests/ref_collide.py against each other and on hand-derived cases, and the kernels' per-body code (csrc/vxrt_collide.hpp)
compiled for the host (tests/tools/collide_check.cpp) against them, bit for bit, with every table index it forms checked."""
import ctypes as C

import numpy as np
import pytest

from tests import ref_collide as R
from tests.helpers import build_harness, float_bits, run_harness_files

F = np.float32
YXZ, XYZ = (1, 0, 2), (0, 1, 2)


def _body(lo, hi, d=(0, 0, 0)):
    return np.asarray([*lo, *hi, *d], F)


def _both(vox, bodies, order=YXZ):
    """move and overlap results of both restatements, asserted equal; returns the vectorised ones"""
    b = np.asarray(bodies, F).reshape(-1, 9)
    mv, ms = R.move_boxes(vox, b, order), R.move_boxes_scalar(vox, b, order)
    assert np.array_equal(float_bits(mv[0]), float_bits(ms[0])) and np.array_equal(mv[1], ms[1])
    ov, os_ = R.overlap_boxes(vox, b), R.overlap_boxes_scalar(vox, b)
    assert np.array_equal(ov[0], os_[0]) and np.array_equal(ov[1], os_[1])
    return mv, ov


def _world():
    v = np.zeros((16, 16, 16), bool)
    v[:, 3, :] = True  # a floor: top face at y = 4
    return v


def _bits_equal(got, want):
    return np.array_equal(float_bits(np.asarray(got, F)), float_bits(np.asarray(want, F)))


def test_fall_onto_a_floor_snaps_to_the_face():
    vox = _world()
    (lohi, fl), _ = _both(vox, [_body((4.2, 6.5, 4.2), (5.0, 8.3, 5.0), (0, -5, 0))])
    assert fl[0] == 2
    assert lohi[0, 1] == F(4.0)  # exactly the floor's top face
    assert _bits_equal(lohi[0, 4], F(F(8.3) + F(F(4.0) - F(6.5))))
    assert _bits_equal(lohi[0, [0, 2, 3, 5]], F([4.2, 4.2, 5.0, 5.0]))
    # upward into a ceiling: hi snaps to the ceiling's lower face
    vox[:, 12, :] = True
    (lohi, fl), _ = _both(vox, [_body((4.2, 6.5, 4.2), (5.0, 8.3, 5.0), (0, 7.25, 0))])
    assert fl[0] == 2 and lohi[0, 4] == F(12.0) and _bits_equal(lohi[0, 1], F(F(6.5) + F(F(12.0) - F(8.3))))


def test_body_resting_on_a_face_stays_put():
    vox = _world()
    b = _body((4.2, 4.0, 4.2), (5.0, 5.8, 5.0), (0, -0.5, 0))
    (lohi, fl), (cnt, _) = _both(vox, [b])
    assert fl[0] == 2 and _bits_equal(lohi[0], b[:6])
    assert cnt[0] == 0  # resting on the face does not overlap the floor


def test_sliding_along_a_wall_whose_faces_only_touch():
    vox = _world()
    vox[8, :, :] = True  # a wall: faces at x = 8 and x = 9
    b = _body((6.0, 4.0, 2.0), (8.0, 6.0, 3.0), (0, 0, 3.5))
    (lohi, fl), (cnt, _) = _both(vox, [b])
    assert fl[0] == 0 and cnt[0] == 0
    assert _bits_equal(lohi[0], [6.0, 4.0, 5.5, 8.0, 6.0, 6.5])
    # pushing into it is blocked with no move
    (lohi, fl), _ = _both(vox, [_body((6.0, 4.0, 2.0), (8.0, 6.0, 3.0), (0.25, 0, 0))])
    assert fl[0] == 1 and _bits_equal(lohi[0], [6.0, 4.0, 2.0, 8.0, 6.0, 3.0])


def test_a_step_of_five_does_not_jump_a_one_voxel_wall():
    vox = _world()
    vox[8, 4:, :] = True  # voxel 7 is the gap in front of a one-voxel wall
    (lohi, fl), _ = _both(vox, [_body((5.5, 4.0, 2.0), (6.5, 6.0, 3.0), (5, 0, 0))])
    assert fl[0] == 1 and lohi[0, 3] == F(8.0) and lohi[0, 0] == F(7.0)
    (lohi, fl), _ = _both(vox, [_body((10.5, 4.0, 2.0), (11.5, 6.0, 3.0), (-5, 0, 0))])  # from the other side
    assert fl[0] == 1 and lohi[0, 0] == F(9.0) and lohi[0, 3] == F(10.0)


def test_a_body_inside_solid_moves_out():
    vox = np.zeros((16, 16, 16), bool)
    vox[4:7, 4:7, 4:7] = True
    b = _body((5.2, 5.2, 5.2), (6.8, 6.8, 6.8), (0, 5, 0))
    (lohi, fl), (cnt, _) = _both(vox, [b])
    assert cnt[0] == 8  # voxels 5, 6 on each axis
    assert fl[0] == 0 and _bits_equal(lohi[0], [5.2, F(5.2) + F(5), 5.2, 6.8, F(6.8) + F(5), 6.8])


def test_a_body_falls_off_the_world_edge():
    vox = _world()
    b = _body((-3.0, 10.0, 5.0), (-1.0, 12.0, 6.0), (0, -20, 0))  # beside the world: nothing below
    (lohi, fl), _ = _both(vox, [b])
    assert fl[0] == 0 and _bits_equal(lohi[0], [-3.0, -10.0, 5.0, -1.0, -8.0, 6.0])
    b = _body((-0.5, 10.0, 5.0), (0.5, 12.0, 6.0), (0, -20, 0))  # half over the edge: lands on the floor
    (lohi, fl), _ = _both(vox, [b])
    assert fl[0] == 2 and lohi[0, 1] == F(4.0)
    b = _body((1.0, 4.0, 5.0), (3.0, 5.5, 6.0), (0, 0, 30))  # walks off the far face of the world
    (lohi, fl), _ = _both(vox, [b])
    assert fl[0] == 0 and lohi[0, 2] == F(35.0)


def test_corner_step_depends_on_the_order():
    vox = _world()
    vox[8:, 4, :] = True  # a step of one voxel at x >= 8
    b = _body((6.5, 5.5, 4.2), (7.5, 7.5, 5.0), (2, -1, 0))
    (yxz, fy), _ = _both(vox, [b], YXZ)
    (xyz, fx), _ = _both(vox, [b], XYZ)
    assert fy[0] == 1 and _bits_equal(yxz[0], [7.0, 4.5, 4.2, 8.0, 6.5, 5.0])  # down first, then stopped by the step
    assert fx[0] == 2 and _bits_equal(xyz[0], [8.5, 5.0, 4.2, 9.5, 7.0, 5.0])  # across first, then onto the step


def test_zero_and_negative_zero_steps_do_nothing():
    vox = _world()
    bodies = [_body((4.2, 3.5, 4.2), (5.0, 5.0, 5.0), (z, z, z)) for z in (F(0.0), F(-0.0))]  # inside the floor
    (lohi, fl), _ = _both(vox, bodies)
    assert list(fl) == [0, 0]
    for i in range(2):
        assert _bits_equal(lohi[i], bodies[i][:6])


def test_invalid_bodies():
    vox = _world()
    ok = _body((2.0, 5.0, 2.0), (3.0, 7.0, 3.0), (0.5, -0.5, 0.25))
    up = np.nextafter(F(64), F(np.inf))
    cases = []
    for k in range(9):
        for v in (np.nan, np.inf, -np.inf):
            b = ok.copy()
            b[k] = v
            cases.append((b, False))
    for k in range(3):
        b = ok.copy()
        b[3 + k] = b[k]  # lo == hi
        cases.append((b, False))
        b = ok.copy()
        b[3 + k] = b[k] - 1  # lo > hi
        cases.append((b, False))
        b = ok.copy()
        b[3 + k] = b[k] + 64  # extent 64: valid
        cases.append((b, True))
        b = ok.copy()
        b[k], b[3 + k] = F(0.5), F(0.5) + up  # extent just above 64
        cases.append((b, False))
        for dv, good in ((64.0, True), (-64.0, True), (up, False), (-up, False)):
            b = ok.copy()
            b[6 + k] = dv
            cases.append((b, good))
        for lo, hi, good in ((2.0 ** 24 - 2, 2.0 ** 24 - 1, True), (2.0 ** 24 - 1, 2.0 ** 24, False),
                             (-2.0 ** 24, -2.0 ** 24 + 1, False), (-2.0 ** 24 + 1, -2.0 ** 24 + 3, True)):
            b = ok.copy()
            b[k], b[3 + k] = lo, hi
            cases.append((b, good))
    bodies = np.stack([c[0] for c in cases])
    want = np.asarray([c[1] for c in cases])
    assert np.array_equal(R.valid(bodies), want)
    (lohi, fl), (cnt, ofl) = _both(vox, bodies)
    bad = ~want
    assert np.all(fl[bad] == R.INVALID) and np.all(ofl[bad] == R.INVALID) and np.all(cnt[bad] == 0)
    assert np.array_equal(float_bits(lohi[bad]), float_bits(bodies[bad, :6]))  # returned unchanged
    assert not np.any(fl[want] & R.INVALID) and not np.any(ofl[want])


def test_overlap_counts_by_hand():
    vox = _world()
    vox[5, 5, 5] = True
    b = [_body((0, 0, 0), (16, 16, 16)), _body((4.9, 4.9, 4.9), (5.1, 5.1, 5.1)), _body((5, 4, 5), (6, 5, 6)),
         _body((-10, 3.5, -10), (30, 3.6, 30)), _body((6, 6, 6), (6.5, 9, 9))]
    _, (cnt, fl) = _both(vox, b)
    assert list(cnt) == [257, 1, 0, 256, 0] and list(fl) == [0] * 5


@pytest.mark.parametrize("seed", range(4))
def test_the_two_restatements_agree_on_random_cases(seed):
    rng = np.random.default_rng(100 + seed)
    vox = rng.random((24, 16, 24)) < [0.05, 0.2, 0.4, 0.1][seed]
    vox[:, 2, :] |= seed % 2 == 0
    b = R.random_bodies(rng, vox.shape, 300, small=True)
    for order in (YXZ, XYZ, (2, 0, 1)):
        (lohi, fl), _ = _both(vox, b, order)
    assert np.count_nonzero(fl & 7) > 20 and np.count_nonzero(fl == 0) > 20


# ---- the kernels' per-body code on the host --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "collide_check")


def _run_harness(harness, tmp_path, vox, bodies, factor, order):
    from oracle import vxo
    X, Y, Z = vox.shape
    b = np.ascontiguousarray(bodies, F)
    n = len(b)
    raw, stdout = run_harness_files(harness, tmp_path, [factor, X, Y, Z, n, *order], vxo.dense_from_voxels(vox), b)
    raw = raw.view(np.uint32)
    lohi = raw[: 6 * n].view(F).reshape(n, 6)
    mf, cnt, of = raw[6 * n: 7 * n], raw[7 * n: 8 * n], raw[8 * n: 9 * n]
    return lohi, mf, cnt, of, stdout


def test_host_code_on_the_hand_derived_cases(harness, tmp_path):
    vox = np.zeros((64, 64, 64), bool)  # the hand-derived world in a corner of one the brickmap builder takes at f = 8
    vox[:16, :16, :16] = _world()
    vox[8:16, 4, :16] = True
    b = np.stack([_body((4.2, 6.5, 4.2), (5.0, 8.3, 5.0), (0, -5, 0)), _body((4.2, 4.0, 4.2), (5.0, 5.8, 5.0), (0, -0.5, 0)),
                  _body((6.5, 5.5, 4.2), (7.5, 7.5, 5.0), (2, -1, 0)), _body((-3.0, 10.0, 5.0), (-1.0, 12.0, 6.0), (0, -20, 0)),
                  _body((4.2, 3.5, 4.2), (5.0, 5.0, 5.0), (-0.0, -0.0, -0.0)), _body((1, 1, 1), (0, 2, 2), (0, 0, 0))])
    for order in (YXZ, XYZ):
        lohi, mf, cnt, of, _ = _run_harness(harness, tmp_path, vox, b, 8, order)
        (wl, wf), (wc, wo) = _both(vox, b, order)
        assert np.array_equal(float_bits(lohi), float_bits(wl)) and np.array_equal(mf, wf)
        assert np.array_equal(cnt, wc) and np.array_equal(of, wo)


@pytest.mark.parametrize("factor,dims,density,n", [(8, (64, 64, 64), 0.05, 4000), (16, (128, 128, 128), 0.02, 3000),
                                                   (32, (256, 256, 256), 0.01, 2000), (8, (8192, 64, 64), 0.02, 3000)])
def test_host_code_equals_the_reference_on_random_worlds(harness, tmp_path, factor, dims, density, n):
    """move (three orders) and overlap of random bodies -- limits, bodies half outside the world, invalid ones included --
    on random worlds at f = 8, 16, 32 and a wide grid: bit-equal to the reference, every gather inside the tables"""
    rng = np.random.default_rng(factor + dims[0])
    vox = rng.random(dims) < density
    vox[:, dims[1] // 4, :] |= rng.random((dims[0], dims[2])) < 0.7  # a holed floor
    b = R.random_bodies(rng, dims, n)
    for order in (YXZ, XYZ, (2, 1, 0)):
        lohi, mf, cnt, of, out = _run_harness(harness, tmp_path, vox, b, factor, order)
        wl, wf = R.move_boxes(vox, b, order)
        wc, wo = R.overlap_boxes(vox, b)
        assert np.array_equal(float_bits(lohi), float_bits(wl)), np.flatnonzero((float_bits(lohi) != float_bits(wl)).any(1))[:10]
        assert np.array_equal(mf, wf) and np.array_equal(cnt, wc) and np.array_equal(of, wo)
        assert np.count_nonzero(wf & 7) > n // 20 and np.count_nonzero(wf == R.INVALID) > 0 and wc.max() > 0


def test_collide_symbols_exported():
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_move_boxes", "vxrt_overlap_boxes", "vxrt_move_boxes_host", "vxrt_overlap_boxes_host"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    order = (C.c_int32 * 3)(1, 0, 2)
    assert lib.vxrt_move_boxes(None, None, 1, order, None, None, None) == -1
    assert lib.vxrt_overlap_boxes(None, None, 1, None, None, None) == -1
    assert lib.vxrt_move_boxes_host(None, None, 1, order, None, None) == -1
    assert lib.vxrt_overlap_boxes_host(None, None, 1, None, None) == -1
    assert vx.Body.pack([vx.Body((0, 0, 0), (1, 2, 1), (0, -1, 0))]).tolist() == [[0, 0, 0, 1, 2, 1, 0, -1, 0]]
    assert (vx.BODY_BLOCKED_X, vx.BODY_BLOCKED_Y, vx.BODY_BLOCKED_Z, vx.BODY_INVALID) == (1, 2, 4, 8)
