"""Voxel editing (include/vxrt.h, vxrt_edit_voxels) without a GPU: the oracle's two restatements of the edit semantics
(C: oracle/vxo_edit.c vxo_apply_edits; numpy: oracle/ref_edit.py apply_edits) on hand-derived cases and against each other,
the per-brick edit logic and the slot plan of the library (voxelengine_amd/csrc/vxrt_edit.hpp) compiled for the host and
held against the oracle, and the new ABI symbols."""

import numpy as np
import pytest

from tests.helpers import build_harness, run_harness

BOX, SPHERE = 0, 1


def _both(vxo, vox, ops):
    """the C restatement (on dense tiled words) and the numpy one (on the bool grid); asserted equal"""
    from oracle import ref_edit, vxo_edit
    X, Y, Z = vox.shape
    c = vxo_edit.voxels_from_dense(vxo_edit.apply_edits(vxo.dense_from_voxels(vox), X, Y, Z, ops), X, Y, Z)
    p = ref_edit.apply_edits(vox, ops)
    assert np.array_equal(c, p)
    return c


def test_sphere_voxel_counts(vxo):
    empty = np.zeros((16, 16, 16), bool)
    for r, n in [(0, 1), (1, 7), (2, 33)]:
        v = _both(vxo, empty, [(SPHERE, 1, (8, 8, 8), (r, 0, 0))])
        assert v.sum() == n, r
        assert v[8, 8, 8]
    assert _both(vxo, empty, [(SPHERE, 1, (0, 0, 0), (1, 0, 0))]).sum() == 4   # clipped at the corner: centre + 3 axes


def test_box_crossing_every_face_is_clipped(vxo):
    empty = np.zeros((16, 24, 32), bool)
    v = _both(vxo, empty, [(BOX, 1, (-5, -100, -1), (3, 30, 40))])
    want = np.zeros_like(empty)
    want[0:4, :, :] = True
    assert np.array_equal(v, want)
    v = _both(vxo, empty, [(BOX, 1, (-2147483648, -2147483648, -2147483648), (2147483647, 2147483647, 2147483647))])
    assert v.all()


def test_set_and_clear_order(vxo):
    empty = np.zeros((16, 16, 16), bool)
    a = (BOX, 1, (2, 2, 2), (9, 9, 9))
    b = (SPHERE, 0, (8, 8, 8), (4, 0, 0))
    set_clear = _both(vxo, empty, [a, (b[0], 0, b[2], b[3])])
    clear_set = _both(vxo, empty, [(b[0], 0, b[2], b[3]), a])
    overlap = _both(vxo, empty, [a]) & _both(vxo, empty, [(SPHERE, 1, (8, 8, 8), (4, 0, 0))])
    assert overlap.sum() > 0
    assert not set_clear[overlap].any() and clear_set[overlap].all()      # the last op wins on the overlap
    assert np.array_equal(set_clear | overlap, clear_set)


def test_shapes_outside_change_nothing(vxo):
    rng = np.random.default_rng(1)
    vox = rng.random((16, 16, 16)) < 0.3
    ops = [(BOX, 1, (16, 0, 0), (40, 15, 15)), (BOX, 0, (0, -9, 0), (15, -1, 15)), (BOX, 1, (5, 5, 5), (4, 9, 9)),
           (SPHERE, 0, (-3, 8, 8), (2, 0, 0)), (SPHERE, 1, (40, 40, 40), (20, 0, 0))]
    assert np.array_equal(_both(vxo, vox, ops), vox)


def test_invalid_ops_are_refused(vxo):
    from oracle import ref_edit, vxo_edit
    vox = np.zeros((8, 8, 8), bool)
    for bad in [(2, 1, (0, 0, 0), (1, 1, 1)), (BOX, 2, (0, 0, 0), (1, 1, 1)), (SPHERE, 1, (4, 4, 4), (-1, 0, 0)),
                (SPHERE, 1, (4, 4, 4), (1, 1, 0)), (SPHERE, 0, (4, 4, 4), (1, 0, 2))]:
        with pytest.raises(ValueError):
            vxo_edit.apply_edits(vxo.dense_from_voxels(vox), 8, 8, 8, [(BOX, 1, (0, 0, 0), (7, 7, 7)), bad])
        with pytest.raises(ValueError):
            ref_edit.apply_edits(vox, [(BOX, 1, (0, 0, 0), (7, 7, 7)), bad])


def random_ops(rng, dims, n):
    ops = []
    for _ in range(n):
        if rng.random() < 0.5:
            lo = [int(rng.integers(-8, d + 8)) for d in dims]
            ops.append((BOX, int(rng.integers(0, 2)), lo, [l + int(rng.integers(-2, d // 2)) for l, d in zip(lo, dims)]))
        else:
            c = [int(rng.integers(-10, d + 10)) for d in dims]
            ops.append((SPHERE, int(rng.integers(0, 2)), c, (int(rng.integers(0, max(dims) // 3)), 0, 0)))
    return ops


def test_c_and_numpy_restatements_agree(vxo):
    rng = np.random.default_rng(7)
    for i in range(2000):
        vox = rng.random((64, 64, 64)) < (0.0 if i % 3 == 0 else 0.1)
        _both(vxo, vox, random_ops(rng, (64, 64, 64), int(rng.integers(0, 9))))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "edit_check", "vxo_edit.c")


@pytest.mark.parametrize("factor,edge,rounds", [(8, 64, 12), (16, 128, 4), (32, 256, 2)])
def test_host_brick_logic_equals_the_oracle(harness, factor, edge, rounds):
    """k_edit_bricks' functions (op filter from the last covering op, membership, extents) brick by brick: images and
    packed extents equal the oracle's rebuilt brickmap of the edited dense grid, for every brick of random worlds."""
    out = run_harness(harness, "bricks", factor, edge, rounds)
    changed = int(out.split(" changed")[0].split()[-1])
    assert changed > 0


def test_host_slot_plan(harness):
    """Deterministic slot assignment: frees first, the lowest free slot next, growth of the high-water mark only when the
    free list is exhausted; the growth rule (1.5x or what is needed); validation and clipping of ops."""
    run_harness(harness, "plan")


def test_edit_symbols_exported():
    import voxelengine_amd as vx
    lib = vx.load()
    for name in ("vxrt_edit_voxels", "vxrt_edit_reserve"):
        assert name in vx.EXPORTS and hasattr(lib, name)
    assert lib.vxrt_abi_version() == 3
    # no context: refused before anything else
    assert lib.vxrt_edit_voxels(None, None, 0, None) == -1
    assert lib.vxrt_edit_reserve(None, 10) == -1
    op = vx.EditSphere((1, 2, 3), 4, 0)
    assert (op.kind, op.value, list(op.a), list(op.b)) == (vx.EDIT_SPHERE, 0, [1, 2, 3], [4, 0, 0])
