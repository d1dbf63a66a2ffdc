"""ctypes binding of the C ORACLE of the voxel edits (oracle/vxo_edit.c, built on its own into oracle/libvxo_edit.so).

TEST INFRASTRUCTURE ONLY (like the rest of oracle/): imported by tests/ and tools/ alone.  The reference for an edited
world is ``vxo.World.from_dense(apply_edits(dense, X, Y, Z, ops), X, Y, Z, factor)``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
BOX, SPHERE = 0, 1


class EditOp(C.Structure):
    """vxo_edit_op (= vxrt_edit_op): kind 0 = box a..b inclusive, 1 = sphere centre a, radius b[0]; value 1 = set, 0 = clear."""
    _fields_ = [("kind", C.c_int32), ("value", C.c_int32), ("a", C.c_int32 * 3), ("b", C.c_int32 * 3)]


def build(force: bool = False) -> str:
    """gcc with the oracle's IEEE flags (oracle/Makefile); rebuilt when the sources are newer than the library."""
    so = os.path.join(_HERE, "libvxo_edit.so")
    srcs = [os.path.join(_HERE, f) for f in ("vxo_edit.c", "vxo_edit.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(_HERE, "libvxo_edit.tmp%d.so" % os.getpid())
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                               "-shared", "-o", tmp, srcs[0]])
        os.replace(tmp, so)
    return so


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        L = C.CDLL(build())
        L.vxo_apply_edits.restype = C.c_int
        L.vxo_apply_edits.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(EditOp), C.c_size_t]
        _LIB = L
    return _LIB


def _as_op(o) -> EditOp:
    kind, value, a, b = o if isinstance(o, tuple) else (o.kind, o.value, o.a, o.b)
    e = EditOp()
    e.kind, e.value = int(kind), int(value)
    e.a = (C.c_int32 * 3)(*[int(v) for v in a])
    e.b = (C.c_int32 * 3)(*[int(v) for v in b])
    return e


def apply_edits(dense_words: np.ndarray, X: int, Y: int, Z: int, ops) -> np.ndarray:
    """vxo_apply_edits on a COPY of dense tiled-linear bit words; ops are (kind, value, a, b) tuples or objects with those
    attributes.  Raises ValueError on an invalid op."""
    out = np.array(dense_words, np.uint32, copy=True)
    ops = [_as_op(o) for o in ops]
    arr = (EditOp * max(len(ops), 1))(*ops)
    if lib().vxo_apply_edits(out.ctypes.data, X, Y, Z, arr, len(ops)) != 0:
        raise ValueError("invalid edit op")
    return out


def voxels_from_dense(words: np.ndarray, X: int, Y: int, Z: int) -> np.ndarray:
    """tiled-linear bit words -> bool [x, y, z] (inverse of vxo.dense_from_voxels)."""
    bits = np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")[: X * Y * Z]
    v = bits.astype(bool).reshape(Z // 8, Y // 8, X // 8, 8, 8, 8)
    return v.transpose(2, 5, 1, 4, 0, 3).reshape(X, Y, Z)
