"""ctypes binding of the C ORACLE of the region readback and voxel stamps (oracle/vxo_region.c, built on its own into
oracle/libvxo_region.so).

TEST INFRASTRUCTURE ONLY (like the rest of oracle/): imported by tests/ and tools/ alone.  The reference for a stamped
world is ``vxo.World.from_dense(apply_stamps(dense, X, Y, Z, stamps), X, Y, Z, factor)``; stamps are (origin, words, dims,
mode) tuples with the words in the region layout (oracle/vxo_region.h).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
REPLACE, UNION, SUBTRACT = 0, 1, 2


class Stamp(C.Structure):
    """vxo_stamp (= vxrt_stamp, with host bits)"""
    _fields_ = [("bits", C.c_void_p), ("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("mode", C.c_int32),
                ("reserved", C.c_int32)]


def build(force: bool = False) -> str:
    """gcc with the oracle's IEEE flags (oracle/Makefile); rebuilt when the sources are newer than the library."""
    so = os.path.join(_HERE, "libvxo_region.so")
    srcs = [os.path.join(_HERE, f) for f in ("vxo_region.c", "vxo_region.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(_HERE, "libvxo_region.tmp%d.so" % os.getpid())
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                               "-shared", "-o", tmp, srcs[0]])
        os.replace(tmp, so)
    return so


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        L = C.CDLL(build())
        L.vxo_region_words.restype = C.c_uint64
        L.vxo_region_words.argtypes = [C.POINTER(C.c_int32)]
        L.vxo_read_region.restype = C.c_int
        L.vxo_read_region.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.c_void_p]
        L.vxo_apply_stamps.restype = C.c_int
        L.vxo_apply_stamps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Stamp), C.c_size_t]
        _LIB = L
    return _LIB


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def region_words(dims) -> int:
    return int(lib().vxo_region_words(_i3(dims)))


def read_region(dense_words: np.ndarray, X: int, Y: int, Z: int, origin, dims) -> np.ndarray:
    """vxo_read_region: region words (uint32) of the box origin .. origin + dims - 1 of dense tiled-linear bits."""
    out = np.zeros(max(region_words(dims), 1), np.uint32)
    src = np.ascontiguousarray(dense_words, np.uint32)
    if lib().vxo_read_region(src.ctypes.data, X, Y, Z, _i3(origin), _i3(dims), out.ctypes.data) != 0:
        raise ValueError("invalid region")
    return out[: region_words(dims)]


def apply_stamps(dense_words: np.ndarray, X: int, Y: int, Z: int, stamps) -> np.ndarray:
    """vxo_apply_stamps on a COPY of dense tiled-linear bit words; stamps are (origin, words, dims, mode) tuples (words
    None: a NULL pointer).  Raises ValueError on an invalid stamp."""
    out = np.array(dense_words, np.uint32, copy=True)
    keep, descs = [], []
    for origin, words, dims, mode in stamps:
        s = Stamp()
        if words is not None:
            w = np.ascontiguousarray(words, np.uint32)
            keep.append(w)
            s.bits = w.ctypes.data
        s.origin, s.dims, s.mode, s.reserved = _i3(origin), _i3(dims), int(mode), 0
        descs.append(s)
    arr = (Stamp * max(len(descs), 1))(*descs)
    if lib().vxo_apply_stamps(out.ctypes.data, X, Y, Z, arr, len(descs)) != 0:
        raise ValueError("invalid stamp")
    return out
