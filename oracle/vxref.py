"""ctypes binding of the REFERENCE built as host C++ (oracle/_ref/libvxref_<variant>.so, made by oracle/ref_build.py).

TEST INFRASTRUCTURE ONLY.  Every call runs the reference's own functions (oracle/ref_driver.cpp); the oracle
(oracle/vxo.py) is pinned to them by tests/test_reference_pin.py and the HIP path by tests/test_gpu_reference_parity.py.
Importing this module builds nothing: the libraries come from __graft_entry__.build() (or `python -m oracle.ref_build`)
on a machine that has the reference's sources, and load() raises where they are missing.

One library per variant of the reference's compile-time switches (ref_build.VARIANTS), each loaded RTLD_LOCAL so that
their identically named globals stay apart.  The driver is single-threaded: never call into one library from two threads.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from oracle import ref_build

VARIANTS = tuple(ref_build.VARIANTS)
DEFAULT = "shadow_s1"
_LIBS: dict = {}


def available() -> bool:
    """the libraries are there and not stale (built from the recipe files as they stand)"""
    return ref_build.built()


def reference_present() -> bool:
    return ref_build.reference_dir() is not None


def switches(variant: str) -> dict:
    """the oracle.vxo.make_params keywords (mode, checkerboard, shadow, bounce_samples, ortho) this variant equals"""
    return dict(ref_build.VARIANTS[variant][2])


def load(variant: str = DEFAULT) -> C.CDLL:
    if variant not in _LIBS:
        path = ref_build.lib_path(variant)
        if not ref_build.built():
            raise FileNotFoundError("%s is missing or older than the recipe: run __graft_entry__.build() on a machine with the reference's sources" % path)
        L = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
        vp, sz = C.c_void_p, C.c_size_t
        L.vxref_variant.restype = C.c_char_p
        L.vxref_checkerboard.restype = C.c_int
        L.vxref_sample_index.restype = C.c_uint32
        L.vxref_sample_index.argtypes = [C.c_uint32] * 5
        L.vxref_position_from_index.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_uint32)] * 3
        L.vxref_sample_index_sweep.argtypes = [C.c_uint32] * 3 + [vp, vp]
        L.vxref_ray_aabb.argtypes = [sz] + [vp] * 7
        L.vxref_dda.argtypes = [vp, vp, sz, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int] + [vp] * 7
        L.vxref_world_build.restype = vp
        L.vxref_world_build.argtypes = [vp] + [C.c_int] * 4
        L.vxref_world_free.argtypes = [vp]
        L.vxref_world_tables.argtypes = [vp] * 5
        L.vxref_trace.argtypes = [vp, C.c_int, sz] + [vp] * 6
        L.vxref_render.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp]
        L.vxref_get_directions.argtypes = [vp] * 4
        L.vxref_hash.argtypes = [sz, vp, vp, vp]
        L.vxref_fbm.argtypes = [sz, vp, vp]
        L.vxref_populate.argtypes = [C.c_int] * 3 + [vp]
        assert L.vxref_variant().decode() == variant
        _LIBS[variant] = L
    return _LIBS[variant]


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


# ---- layout
def sample_index(x, y, z, w, h, variant=DEFAULT) -> int:
    return int(load(variant).vxref_sample_index(x, y, z, w, h))


def position_from_index(i, w, h, variant=DEFAULT):
    x, y, z = C.c_uint32(), C.c_uint32(), C.c_uint32()
    load(variant).vxref_position_from_index(i, w, h, C.byref(x), C.byref(y), C.byref(z))
    return x.value, y.value, z.value


def sample_index_sweep(w, h, d, variant=DEFAULT):
    """every index of a w*h*d grid: (positions (n, 3), the index each position maps back to (n,))"""
    n = w * h * d
    pos, back = np.zeros((n, 3), np.uint32), np.zeros(n, np.uint32)
    load(variant).vxref_sample_index_sweep(w, h, d, pos.ctypes.data, back.ctypes.data)
    return pos, back


# ---- ray / box, batched; p and normal are 0 where the reference writes nothing (a miss)
def ray_aabb(start, d, bmin, bmax, variant=DEFAULT):
    s, d, lo, hi = (_f32(a, (-1, 3)) for a in (start, d, bmin, bmax))
    n = len(s)
    hit, p, nrm = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    load(variant).vxref_ray_aabb(n, s.ctypes.data, d.ctypes.data, lo.ctypes.data, hi.ctypes.data, hit.ctypes.data, p.ctypes.data,
                                 nrm.ctypes.data)
    return dict(hit=hit, pos=p, normal=nrm)


def dda(dense_words, dims, start, d, *, region=None, max_steps=2048, cell_boxes=None, cell_boxes_scale=0, take_initial_step=False,
        variant=DEFAULT):
    """the single-level traversal over a dense tiled-linear grid, n rays; fields the reference leaves unwritten are 0"""
    words = np.ascontiguousarray(dense_words, np.uint32)
    s, d = _f32(start, (-1, 3)), _f32(d, (-1, 3))
    n = len(s)
    dm = (C.c_int * 3)(*dims)
    reg = None if region is None else _f32(region, (6,))
    cb = None if cell_boxes is None else _f32(cell_boxes)
    out = dict(hit=np.zeros(n, np.uint8), out_of_bounds=np.zeros(n, np.uint8), steps=np.zeros(n, np.int32),
               hit_cell=np.zeros((n, 3), np.float32), point=np.zeros((n, 3), np.float32), next_cell=np.zeros((n, 3), np.float32),
               normal=np.zeros((n, 3), np.float32))
    load(variant).vxref_dda(words.ctypes.data, C.addressof(dm), n, s.ctypes.data, d.ctypes.data, None if reg is None else reg.ctypes.data,
                            max_steps, None if cb is None else cb.ctypes.data, cell_boxes_scale, int(take_initial_step),
                            *[out[k].ctypes.data for k in ("hit", "out_of_bounds", "steps", "hit_cell", "point", "next_cell", "normal")])
    return out


class World:
    """A brickmap built by the reference's own builder from dense tiled-linear bits; traced and rendered by the
    reference on the host arrays that builder returned."""

    def __init__(self, dense_words, X, Y, Z, factor, variant=DEFAULT):
        assert X * Y * Z <= 256 ** 3, "reference-built worlds stay at or below 256^3 (its builder starts one thread per CPU)"
        self.variant, self._L = variant, load(variant)
        dense_words = np.ascontiguousarray(dense_words, np.uint32)
        assert dense_words.size == X * Y * Z // 32
        self.dense_words = dense_words
        self.dims, self.factor = (X, Y, Z), factor
        self.cdims = (X // factor, Y // factor, Z // factor)
        self.ncells = self.cdims[0] * self.cdims[1] * self.cdims[2]
        self._h = self._L.vxref_world_build(dense_words.ctypes.data, X, Y, Z, factor)

    @staticmethod
    def from_voxels(vox, factor, variant=DEFAULT) -> "World":
        from oracle import vxo
        X, Y, Z = vox.shape
        return World(vxo.dense_from_voxels(vox), X, Y, Z, factor, variant)

    def for_variant(self, variant) -> "World":
        """the same world built again by another variant's library (handles are not shared between libraries)"""
        return self if variant == self.variant else World(self.dense_words, *self.dims, self.factor, variant)

    def __del__(self):
        try:
            if self._h:
                self._L.vxref_world_free(self._h)
        except Exception:
            pass
        self._h = None

    def tables(self):
        """dict(coarse_bits (ncells/32,), bounds (ncells, 6), brick_dims (ncells, 3), bricks (ncells, f^3/32)), cell by cell
        in the coarse grid's tiled-linear order; a brick without bits reads as zeros"""
        bw = self.factor ** 3 // 32
        t = dict(coarse_bits=np.zeros((self.ncells + 31) // 32, np.uint32), bounds=np.zeros((self.ncells, 6), np.float32),
                 brick_dims=np.zeros((self.ncells, 3), np.uint16), bricks=np.zeros((self.ncells, bw), np.uint32))
        self._L.vxref_world_tables(self._h, *[t[k].ctypes.data for k in ("coarse_bits", "bounds", "brick_dims", "bricks")])
        return t

    def engine_tables(self):
        """the tables in the shape of oracle.vxo.World.wrap / Context.upload_world: (factor, cdims, coarse_bits,
        brick_slot, bounds, pool) with pool slots handed out in cell order (the reference has no slot table)"""
        t = self.tables()
        occ = t["brick_dims"][:, 0] != 0
        slot = np.full(self.ncells, 0xFFFFFFFF, np.uint32)
        slot[occ] = np.arange(int(occ.sum()), dtype=np.uint32)
        return self.factor, self.cdims, t["coarse_bits"], slot, t["bounds"], np.ascontiguousarray(t["bricks"][occ]).reshape(-1)

    def trace(self, origins, dirs, max_steps=2048):
        """hit, steps, normal, pos; pos = +inf on a miss, the convention of the reference's batch kernel (and of
        oracle.vxo.World.trace_batch)"""
        o, d = _f32(origins, (-1, 3)), _f32(dirs, (-1, 3))
        n = len(o)
        hit, steps = np.zeros(n, np.uint8), np.zeros(n, np.int32)
        nrm, pos = np.zeros((n, 3), np.float32), np.full((n, 3), np.inf, np.float32)
        self._L.vxref_trace(self._h, max_steps, n, o.ctypes.data, d.ctypes.data, hit.ctypes.data, steps.ctypes.data, nrm.ctypes.data,
                            pos.ctypes.data)
        return dict(hit=hit, steps=steps, normal=nrm, pos=pos)

    def render(self, W, H, frame_number, origin, fwd, up, right, *, fb=None, fov=90.0, ortho_size=(10.0, 10.0), light_dir=None,
               light_color=(2, 2, 2), ambient=(0.5, 0.5, 0.5)):
        """one frame of this variant into fb ((H, W, 4) uint8, BGRA; kept where the launch writes nothing)"""
        if fb is None:
            fb = np.full((H, W, 4), 255, np.uint8)
        assert fb.dtype == np.uint8 and fb.shape == (H, W, 4) and fb.flags.c_contiguous
        if light_dir is None:
            inv = np.float32(1.0) / np.sqrt(np.float32(3.0), dtype=np.float32)
            light_dir = (inv, inv, inv)
        cam = _f32(np.concatenate([_f32(v, (3,)) for v in (origin, fwd, up, right)]))
        env = _f32(np.concatenate([_f32(v, (3,)) for v in (light_dir, light_color, ambient)]))
        osz = _f32(ortho_size, (2,))
        self._L.vxref_render(self._h, W, H, frame_number, float(fov), osz.ctypes.data, cam.ctypes.data, env.ctypes.data, fb.ctypes.data)
        return fb


# ---- small functions
def get_directions(euler, variant=DEFAULT):
    e, f, u, r = _f32(euler, (3,)), np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    load(variant).vxref_get_directions(e.ctypes.data, f.ctypes.data, u.ctypes.data, r.ctypes.data)
    return f, u, r


def hash_and_random(seeds, variant=DEFAULT):
    s = np.ascontiguousarray(seeds, np.uint32)
    h, r = np.zeros(s.size, np.uint32), np.zeros(s.size, np.float32)
    load(variant).vxref_hash(s.size, s.ctypes.data, h.ctypes.data, r.ctypes.data)
    return h, r


def fbm(xyz, variant=DEFAULT):
    p = _f32(xyz, (-1, 3))
    out = np.zeros(len(p), np.float32)
    load(variant).vxref_fbm(len(p), p.ctypes.data, out.ctypes.data)
    return out


def populate(X, Y, Z, variant=DEFAULT):
    """the reference's world generator kernel run once per voxel: dense tiled-linear words"""
    words = np.zeros(X * Y * Z // 32, np.uint32)
    load(variant).vxref_populate(X, Y, Z, words.ctypes.data)
    return words
