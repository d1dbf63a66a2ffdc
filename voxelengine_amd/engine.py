"""Host-side mirror of the reference's VoxelRT interface over the C ABI (include/vxrt.h).

Reference surface (VoxelRT/VolumeRaytracer.cuh:291-377, VoxelRT/Renderer.cuh:39-55):
``VoxelRaytracer3D`` {UploadVoxelBuffer, UploadVoxelBufferDatas, UploadVoxelBufferDataBounds, SetFactor,
Raytrace} and ``Graphics`` {GetDirections, SetEnvironment, SetFOV, SetOrthoWindowSize, RenderScreen}.
Here one :class:`Context` per GPU carries what the reference keeps in process globals, so eight GPUs can
run from eight ranks.  PyTorch only supplies device memory and streams; every pixel and ray is produced by
the HIP kernels in ``csrc/``.  There is no CPU fallback: without libvxrt.so and a GPU these calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from . import _native as N


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _pose(dst, cam) -> None:
    """``cam`` = (origin, fwd, up, right) into the camera pose ``dst`` of a params struct"""
    dst.origin, dst.fwd, dst.up, dst.right = (_f3(v) for v in cam)


def GetDirections(euler):
    """Graphics::GetDirections (VoxelRT/Renderer.cu:27-42). Host math only."""
    f, u, r = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    N.load().vxrt_get_directions(_f3(euler), f, u, r)
    return (np.array(f[:], np.float32), np.array(u[:], np.float32), np.array(r[:], np.float32))


def tile_schedule(width: int, frame_rows, fwd, up, right, fov_deg: float = 90.0, height: int | None = None):
    """Hand-out order of the 8x8 pixel tiles for the persistent render kernel: expected-longest ray chains first,
    so the wave-level tail at the end of a frame is made of cheap tiles.  A function of the camera only: the cost
    proxy is the elevation of the tile's centre ray (rays pointing up leave the grid at once; rays just below the
    horizon travel farthest).  ``frame_rows``: frame row of every launch-grid row (``range(height)`` for an
    unsharded frame).  Returns uint32 numpy array; scheduling only -- results never depend on it."""
    frame_rows = np.asarray(list(frame_rows), np.int64)
    H = int(height if height is not None else (frame_rows.max() + 1 if frame_rows.size else 1))
    ntx, nty = (width + 7) // 8, (len(frame_rows) + 7) // 8
    t = np.tan(np.float64(fov_deg) * 3.1415 / 180.0 / 2.0)
    cx = (np.arange(ntx) * 8 + 4) / width * 2 - 1
    rows_c = frame_rows[np.minimum(np.arange(nty) * 8 + 4, len(frame_rows) - 1)] if len(frame_rows) else np.zeros(0)
    cy = rows_c / H * 2 - 1
    f, u, r = [np.asarray(v, np.float64) for v in (fwd, up, right)]
    d = f[None, None, :] + (cx[None, :, None] * t * (width / H)) * r[None, None, :] + (cy[:, None, None] * t) * u[None, None, :]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    dy = d[..., 1]
    cost = np.where(dy >= 0, 0.0, 1.0 / np.maximum(-dy, 0.02))  # up-pointing: cheap; grazing: expensive (capped)
    return np.argsort(-cost.reshape(-1), kind="stable").astype(np.uint32)


def world_file_info(path: str) -> "N.WorldInfo":
    """Header of a brickmap file written by :meth:`Context.save_world` (needs no GPU)."""
    info = N.WorldInfo()
    N.check(N.load().vxrt_world_file_info(os.fsencode(path), C.byref(info)))
    return info


def compact_rows(height: int, strip_rows: int, strip_count: int, strip_index: int) -> int:
    return int(N.load().vxrt_compact_rows(height, strip_rows, strip_count, strip_index))


@dataclass
class RenderOptions:
    """Run-time forms of the reference's compile-time switches (VoxelRT/Renderer.cu:4-5,102,123)."""
    mode: int = N.MODE_SHADED
    checkerboard: bool = False
    shadow: bool = False
    bounce_samples: int = 0
    bounce_all_hits: bool = False
    bounce_depth: int = 1           # 2: extension beyond the reference (second bounce, include/vxrt.h)
    ortho: bool = False
    frame_number: int = -1          # < 0: context counter with the reference's post-copy increment
    strip_rows: int = 16
    strip_count: int = 1
    strip_index: int = 0
    compact: bool = False
    collect_stats: bool = False
    tile_schedule: bool = True      # persistent kernel: expected-longest tiles first (scheduling only)
    extra: dict = field(default_factory=dict)


class Context:
    """One MI355X: resident brickmap + camera/lighting state + launches."""

    def __init__(self, device: int = 0):
        self._L = N.load()
        h = C.c_void_p()
        N.check(self._L.vxrt_create(device, C.byref(h)))
        self._h = h
        self.device = device
        self.kernel_variant = 4  # the library's default (= 7: persistent wavefronts on the wave-level tracer)

    def close(self):
        if getattr(self, "_h", None):
            self._L.vxrt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- world ----------------------------------------------------------------------------------
    def upload_world(self, factor: int, cdims, coarse_bits, brick_slot, bounds, pool) -> None:
        """UploadVoxelBuffer + UploadVoxelBufferDatas + UploadVoxelBufferDataBounds + SetFactor
        (VoxelRT/VolumeRaytracer.cu:527-572) with the tables as flat host arrays."""
        cb = np.ascontiguousarray(coarse_bits, np.uint32)
        bs = np.ascontiguousarray(brick_slot, np.uint32)
        bd = np.ascontiguousarray(bounds, np.float32)
        pl = np.ascontiguousarray(pool, np.uint32)
        d = N.WorldDesc()
        d.struct_size = C.sizeof(N.WorldDesc)
        d.factor = factor
        d.cdims = (C.c_int32 * 3)(*[int(c) for c in cdims])
        d.nslots = pl.size // (factor ** 3 // 32)
        d.coarse_bits, d.brick_slot, d.bounds = cb.ctypes.data, bs.ctypes.data, bd.ctypes.data
        d.pool = pl.ctypes.data if pl.size else None
        N.check(self._L.vxrt_upload_world(self._h, C.byref(d)))

    def build_world(self, generator: int, X: int, Y: int, Z: int, factor: int) -> "N.WorldInfo":
        """CreateVoxels + GenerateLowresVoxelBuffer on the device, brick by brick."""
        N.check(self._L.vxrt_build_world_procedural(self._h, generator, X, Y, Z, factor))
        return self.world_info()

    def world_info(self) -> "N.WorldInfo":
        info = N.WorldInfo()
        N.check(self._L.vxrt_world_info_get(self._h, C.byref(info)))
        return info

    def save_world(self, path: str) -> None:
        """Write the resident brickmap to a file (format: include/vxrt.h, "brickmap file")."""
        N.check(self._L.vxrt_save_world(self._h, os.fsencode(path)))

    def load_world(self, path: str) -> "N.WorldInfo":
        """Replace the resident brickmap by the one in ``path`` (validated while it streams into HBM)."""
        N.check(self._L.vxrt_load_world(self._h, os.fsencode(path)))
        return self.world_info()

    # ---- chunk streaming (extension, include/vxrt.h) -------------------------------------------------
    def stream_open(self, path: str, pool_capacity_bricks: int) -> "N.WorldInfo":
        """A world whose bricks are read from the brickmap file ``path`` only for the chunks (8x8x8 tiles of coarse
        cells) near a focus point; the pool is a cache of ``pool_capacity_bricks`` bricks.  Empty until ``stream_focus``."""
        N.check(self._L.vxrt_stream_open(self._h, os.fsencode(path), int(pool_capacity_bricks)))
        return self.world_info()

    def stream_focus(self, focus, radius: float) -> "N.StreamStats":
        st = N.StreamStats()
        N.check(self._L.vxrt_stream_focus(self._h, _f3(focus), float(radius), C.byref(st)))
        return st

    def stream_resident(self, n_chunks: int | None = None) -> np.ndarray:
        """One flag per chunk (tile index of the coarse grid): 1 = its bricks are resident.  ``n_chunks``: the number of
        flags to ask for (default: the world's chunk count; the library refuses any other)."""
        info = self.world_info()
        flags = np.zeros(int(info.ncells) // 512 if n_chunks is None else int(n_chunks), np.uint8)
        N.check(self._L.vxrt_stream_resident(self._h, flags.ctypes.data, flags.size))
        return flags

    def stream_close(self) -> None:
        N.check(self._L.vxrt_stream_close(self._h))

    # ---- voxel editing (extension, include/vxrt.h) ---------------------------------------------------------------
    def edit_voxels(self, ops) -> "N.EditStats":
        """Apply a list of box / sphere set and clear ops (EditBox, EditSphere, or (kind, value, a, b) tuples) to the
        resident world, in order: the last op covering a voxel sets it.  Synchronises the device before and after; all or
        nothing on failure.  Returns what the call did to the brick pool."""
        ops = [o if isinstance(o, N.EditOp) else _edit_op(*o) for o in ops]
        arr = (N.EditOp * max(len(ops), 1))(*ops)
        st = N.EditStats()
        N.check(self._L.vxrt_edit_voxels(self._h, arr if ops else None, len(ops), C.byref(st)))
        return st

    def edit_reserve(self, capacity_bricks: int) -> None:
        """Grow the brick pool to at least ``capacity_bricks`` now, so that later edits need no pool copy."""
        N.check(self._L.vxrt_edit_reserve(self._h, int(capacity_bricks)))

    # ---- region readback and voxel stamps (extension, include/vxrt.h) ----------------------------------------------
    def read_region(self, origin, dims, out=None, stream: int | None = None):
        """The voxels of the box ``origin`` .. ``origin + dims - 1`` as region words (include/vxrt.h: x in 32-bit words,
        rows y fastest, then z; voxels outside the world read 0) in a device tensor of ``region_words(dims)`` int32 (the
        bits of uint32 words), or into ``out``.  Asynchronous on ``stream`` (default: torch's current stream)."""
        call = _Call(self, stream)
        n = region_words(dims)
        out = call.out(n, 4, call.torch.int32, out, "out: a contiguous device tensor of at least region_words(dims) words",
                       any_size=True)
        call.launch(self._L.vxrt_read_region, _i3(origin), _i3(dims), _ptr(out))
        return out[:n] if out.dim() == 1 and out.element_size() == 4 else out

    def read_region_host(self, origin, dims) -> np.ndarray:
        """The voxels of the box ``origin`` .. ``origin + dims - 1`` as a bool [x, y, z] numpy grid (synchronous)."""
        words = np.empty(max(region_words(dims), 1), np.uint32)
        N.check(self._L.vxrt_read_region_host(self._h, _i3(origin), _i3(dims), words.ctypes.data))
        return unpack_region(words, dims)

    def edit_stamps(self, stamps) -> "N.EditStats":
        """Write a list of Stamp(origin, bits, mode) into the resident world in order: the last stamp covering a voxel
        decides it (include/vxrt.h).  ``bits``: a device tensor of region words, or a bool [x, y, z] numpy grid (packed
        and copied to the device here).  Synchronises the device before and after; all or nothing on failure."""
        import torch
        keep, descs = [], []
        for s in stamps:
            bits, dims = s.bits, s.dims
            if isinstance(bits, np.ndarray):
                dims = tuple(int(v) for v in bits.shape) if dims is None else dims
                bits = torch.from_numpy(pack_region(bits).view(np.int32)).to("cuda:%d" % self.device)
            elif dims is None:
                raise ValueError("a stamp of device words needs its dims")
            keep.append(bits)
            d = N.StampDesc()
            d.d_bits = _ptr(bits)
            d.origin = _i3(s.origin)
            d.dims = _i3(dims)
            d.mode = int(s.mode)
            d.reserved = 0
            descs.append(d)
        arr = (N.StampDesc * max(len(descs), 1))(*descs)
        st = N.EditStats()
        N.check(self._L.vxrt_edit_stamps(self._h, arr if descs else None, len(descs), C.byref(st)))
        del keep
        return st

    # ---- box collision queries (extension, include/vxrt.h) -----------------------------------------------------------
    def move_boxes(self, bodies, order=(1, 0, 2), stream: int | None = None):
        """Move boxes through the resident world axis by axis in ``order`` (default y, x, z), stopping each axis at the
        first solid voxel its leading face would enter (include/vxrt.h, vxrt_move_boxes).  ``bodies``: (n, 9) float32 rows
        lo[3], hi[3], delta[3] -- a cuda tensor (asynchronous on ``stream``, default torch's current stream; returns device
        tensors) or a numpy array (the host path, synchronous; returns numpy arrays).  Returns (lohi (n, 6) float32, flags
        (n,) of BODY_BLOCKED_X / _Y / _Z bits, or BODY_INVALID)."""
        order = (C.c_int32 * 3)(*[int(v) for v in order])
        if isinstance(bodies, np.ndarray) or isinstance(bodies, (list, tuple)):
            b = _bodies_np(bodies)
            lohi = np.empty((len(b), 6), np.float32)
            flags = np.empty(len(b), np.uint32)
            N.check(self._L.vxrt_move_boxes_host(self._h, b.ctypes.data, len(b), order, lohi.ctypes.data, flags.ctypes.data))
            return lohi, flags
        call = _Call(self, stream)
        b = call.reads(_bodies_dev(bodies))
        lohi = call.torch.empty((b.shape[0], 6), dtype=call.torch.float32, device=b.device)
        flags = call.torch.empty(b.shape[0], dtype=call.torch.int32, device=b.device)
        call.launch(self._L.vxrt_move_boxes, _ptr(b), b.shape[0], order, _ptr(lohi), _ptr(flags))
        return lohi, flags

    def overlap_boxes(self, bodies, stream: int | None = None):
        """The number of solid voxels each box overlaps (include/vxrt.h, vxrt_overlap_boxes; delta ignored).  ``bodies`` as
        for move_boxes.  Returns (counts (n,), flags (n,): 0, or BODY_INVALID with count 0)."""
        if isinstance(bodies, np.ndarray) or isinstance(bodies, (list, tuple)):
            b = _bodies_np(bodies)
            counts = np.empty(len(b), np.uint32)
            flags = np.empty(len(b), np.uint32)
            N.check(self._L.vxrt_overlap_boxes_host(self._h, b.ctypes.data, len(b), counts.ctypes.data, flags.ctypes.data))
            return counts, flags
        call = _Call(self, stream)
        b = call.reads(_bodies_dev(bodies))
        counts = call.torch.empty(b.shape[0], dtype=call.torch.int32, device=b.device)
        flags = call.torch.empty(b.shape[0], dtype=call.torch.int32, device=b.device)
        call.launch(self._L.vxrt_overlap_boxes, _ptr(b), b.shape[0], _ptr(counts), _ptr(flags))
        return counts, flags

    # ---- floating islands (extension, include/vxrt.h) ----------------------------------------------------------------
    def find_islands(self, origin, dims, anchors: int = N.ISLAND_ANCHOR_FACES | N.ISLAND_ANCHOR_FLOOR, labels: bool = False,
                     max_islands: int = 4096, stream: int | None = None) -> "Islands":
        """The 6-connected components of the solid voxels of the box ``origin`` .. ``origin + dims - 1`` that touch no anchor
        (include/vxrt.h, vxrt_find_islands: by default the box's six faces and world y = 0).  Runs on ``stream`` (default:
        torch's current stream) and waits for it to return the table and the summary.  Returns an Islands: the island
        voxels as device region words (a subtract stamp at ``origin``), the per-voxel component ids when ``labels``, and
        up to ``max_islands`` table rows in ascending id."""
        call = _Call(self, stream)
        i32 = call.torch.int32
        origin, dims = _box(origin, dims)
        ws = int(self._L.vxrt_islands_workspace_bytes(_i3(dims)))
        nvox, nw = _counts(dims, ws)
        work = call.work(ws)
        floating = call.out(nw, 4, i32)
        lab = call.out(nvox, 4, i32) if labels else None
        table = call.out(8 * max(int(max_islands), 1), 4, i32).view(-1, 8)
        summary = call.summary(3)
        call.launch(self._L.vxrt_find_islands, _i3(origin), _i3(dims), int(anchors), _ptr(work), _ptr(floating), _ptr(lab),
                    _ptr(table), int(max_islands), _ptr(summary))
        call.stream.synchronize()
        comps, islands, voxels = (int(v) for v in summary.cpu().numpy().view(np.uint32))
        rows = table[: min(islands, int(max_islands))].cpu().numpy()
        return Islands(origin=origin, dims=dims, floating=floating[:nw], labels=lab[:nvox] if labels else None,
                       table=_island_table(rows), summary=IslandSummary(comps, islands, voxels))

    def find_islands_host(self, origin, dims, anchors: int = N.ISLAND_ANCHOR_FACES | N.ISLAND_ANCHOR_FLOOR,
                          labels: bool = False, max_islands: int = 4096) -> "Islands":
        """find_islands through the synchronous host call (vxrt_find_islands_host): numpy outputs, floating as a bool
        [x, y, z] grid and labels as uint32 [x, y, z]."""
        origin, dims = _box(origin, dims)
        nvox, n = _counts(dims, region_words(dims))
        floating = np.zeros(max(n, 1), np.uint32)
        lab = np.zeros(max(nvox, 1), np.uint32) if labels else None
        table = np.zeros((max(int(max_islands), 1), 8), np.int32)
        summary = np.zeros(3, np.uint32)
        N.check(self._L.vxrt_find_islands_host(self._h, _i3(origin), _i3(dims), int(anchors), floating.ctypes.data,
                                               lab.ctypes.data if labels else None, table.ctypes.data, int(max_islands),
                                               summary.ctypes.data))
        comps, islands, voxels = (int(v) for v in summary)
        return Islands(origin=origin, dims=dims, floating=unpack_region(floating, dims), labels=_grid(lab, dims) if labels else None,
                       table=_island_table(table[: min(islands, int(max_islands))]),
                       summary=IslandSummary(comps, islands, voxels))

    def collapse_islands(self, origin, dims, anchors: int = N.ISLAND_ANCHOR_FACES | N.ISLAND_ANCHOR_FLOOR,
                         max_islands: int = 4096):
        """find_islands, then one STAMP_SUBTRACT edit_stamps of its floating voxels at ``origin``: the islands are deleted.
        Returns (Islands, EditStats)."""
        isl = self.find_islands(origin, dims, anchors, max_islands=max_islands)
        st = self.edit_stamps([Stamp(isl.origin, isl.floating, N.STAMP_SUBTRACT, isl.dims)])
        return isl, st

    # ---- voxel piece queries (extension, include/vxrt.h) -------------------------------------------------------------
    def _piece_descs(self, pieces, call: "_Call | None"):
        """(keep-alive list, PieceDesc array) of Piece objects: device words, kept alive by ``call``, for place_pieces; host
        words (``call`` None) for the _host call"""
        keep, descs = [], []
        for p in pieces:
            bits, dims = p.bits, p.dims
            if isinstance(bits, np.ndarray) and bits.dtype == bool:
                dims = _ints(bits.shape) if dims is None else dims
                bits = pack_region(bits)
            elif dims is None:
                raise ValueError("a piece of region words needs its dims")
            if call is None and hasattr(bits, "cpu"):
                bits = bits.cpu().numpy()
            if isinstance(bits, np.ndarray):
                bits = np.ascontiguousarray(bits).view(np.uint32)
            words = bits.size if isinstance(bits, np.ndarray) else bits.numel() * bits.element_size() // 4
            if words < region_words(dims):
                raise ValueError("a piece holds fewer than region_words(dims) words")
            d = N.PieceDesc()
            if call is None:
                d.d_bits = bits.ctypes.data
            else:
                d.d_bits = _ptr(call.upload(bits) if isinstance(bits, np.ndarray) else call.reads(bits))
            keep.append(bits)
            d.dims = _i3(dims)
            d.reserved = 0
            descs.append(d)
        return keep, (N.PieceDesc * max(len(descs), 1))(*descs)

    def place_pieces(self, pieces, placements, stream: int | None = None):
        """Place rigid pieces against the resident world (include/vxrt.h, vxrt_place_pieces): per placement the solid voxels
        the piece overlaps at its origin, and how far it travels along one axis before it first overlaps.  ``pieces``: up to
        PLACE_MAX_PIECES Piece objects; ``placements``: an (n, 6) int32 cuda tensor of rows piece, origin[3], axis, dist, or
        a list of Placement / an (n, 6) numpy array (copied to the device here).  Asynchronous on ``stream`` (default: torch's
        current stream).  Returns an (n, 4) int32 device tensor of rows overlap, travel, contact, flags (PLACED_BLOCKED,
        PLACED_INVALID).  Torch's allocator keeps the pieces' and placements' device memory from reuse until ``stream`` has
        passed the call, so torch tensors may be dropped as soon as it returns."""
        call = _Call(self, stream)
        torch = call.torch
        if not hasattr(placements, "data_ptr"):
            placements = call.upload(_placements_np(placements))
        if placements.dtype != torch.int32 or placements.dim() != 2 or placements.shape[1] != 6:
            raise ValueError("placements must be an (n, 6) int32 tensor: piece, origin[3], axis, dist")
        pl = call.reads(placements.contiguous())
        _, arr = self._piece_descs(pieces, call)
        out = torch.empty((pl.shape[0], 4), dtype=torch.int32, device=pl.device)
        call.launch(self._L.vxrt_place_pieces, arr if len(pieces) else None, len(pieces), _ptr(pl) if pl.shape[0] else None,
                    pl.shape[0], _ptr(out) if pl.shape[0] else None)
        return out

    def place_pieces_host(self, pieces, placements) -> np.ndarray:
        """place_pieces through the synchronous host call (vxrt_place_pieces_host): numpy in, a PLACED_DTYPE array out."""
        pl = _placements_np(placements)
        keep, arr = self._piece_descs(pieces, None)
        out = np.zeros((len(pl), 4), np.int32)
        N.check(self._L.vxrt_place_pieces_host(self._h, arr if len(pieces) else None, len(pieces), pl.ctypes.data if len(pl) else None,
                                               len(pl), out.ctypes.data if len(pl) else None))
        del keep
        return out.view(PLACED_DTYPE).reshape(-1)

    def drop_islands(self, origin, dims, anchors: int = N.ISLAND_ANCHOR_FACES | N.ISLAND_ANCHOR_FLOOR, max_islands: int = 4096):
        """Let the islands of the box ``origin`` .. ``origin + dims - 1`` fall and land instead of deleting them:
          1. find_islands with labels; 2. if the island table was cut short (more than ``max_islands`` islands) or an island's
          box exceeds the piece limits (PLACE_MAX_DIM per axis, PLACE_MAX_VOXELS), raise ValueError before any change;
          3. one STAMP_SUBTRACT stamp of the floating bits, exactly as collapse_islands; 4. the islands in ascending
          (lo[1], id): the island's piece is the bits of labels == id over its box lo .. hi, placed at lo with axis 1 and
          dist = -min(lo[1], PLACE_MAX_DIST), then written back with one STAMP_UNION stamp at lo + (0, travel, 0).
        Later islands land on earlier ones: a deterministic sequential rule, not a physics engine.  An island that starts
        overlapping one that has already landed merges with it (the sweep ignores the overlap at the start), and the cost
        is one synchronising edit per island.  Returns a DROP_DTYPE array, one row (id, voxels, travel, contact) per island in
        dropping order."""
        import torch
        isl = self.find_islands(origin, dims, anchors, labels=True, max_islands=max_islands)
        if isl.summary.islands > len(isl.table):
            raise ValueError("drop_islands: %d islands, table of %d" % (isl.summary.islands, len(isl.table)))
        for r in isl.table:
            ext = [int(h) - int(l) for l, h in zip(r["lo"], r["hi"])]
            if max(ext) > N.PLACE_MAX_DIM or ext[0] * ext[1] * ext[2] > N.PLACE_MAX_VOXELS:
                raise ValueError("drop_islands: island %d is beyond the piece limits" % int(r["id"]))
        rows = np.zeros(len(isl.table), DROP_DTYPE)
        if not len(isl.table):
            return rows
        self.edit_stamps([Stamp(isl.origin, isl.floating, N.STAMP_SUBTRACT, isl.dims)])
        X, Y, Z = isl.dims
        lab = isl.labels.view(Z, Y, X)
        order = sorted(range(len(isl.table)), key=lambda k: (int(isl.table[k]["lo"][1]), int(isl.table[k]["id"])))
        for n, k in enumerate(order):
            r = isl.table[k]
            lo, hi = [int(v) for v in r["lo"]], [int(v) for v in r["hi"]]
            a = [lo[j] - isl.origin[j] for j in range(3)]
            e = [hi[j] - lo[j] for j in range(3)]
            ident = int(np.uint32(r["id"]).view(np.int32))
            grid = (lab[a[2]: a[2] + e[2], a[1]: a[1] + e[1], a[0]: a[0] + e[0]] == ident).permute(2, 1, 0).cpu().numpy()
            piece = Piece(torch.from_numpy(pack_region(grid).view(np.int32)).to(lab.device), tuple(e))
            res = self.place_pieces([piece], [Placement(0, tuple(lo), 1, -min(lo[1], N.PLACE_MAX_DIST))]).cpu().numpy()[0]
            travel = int(res[1])
            self.edit_stamps([Stamp((lo[0], lo[1] + travel, lo[2]), piece.bits, N.STAMP_UNION, piece.dims)])
            rows[n] = (int(r["id"]), int(r["voxels"]), travel, int(np.int32(res[2]).view(np.uint32)))
        return rows

    # ---- stamp orientations (extension, include/vxrt.h) ---------------------------------------------------------------------
    def transform_stamp(self, bits, dims, orientation: "Orientation", out=None, summary: bool = True, stream: int | None = None):
        """Region words turned or mirrored on the device (include/vxrt.h, vxrt_transform_stamp).  ``bits``: a contiguous device
        tensor of at least region_words(dims) words (a region read, a stamp, a piece, a voxelized mesh, ...); ``orientation``:
        an Orientation.  ``out``: a device tensor of at least region_words(orientation.dims(dims)) words that does not
        overlap ``bits`` (default: a new one).  Asynchronous on ``stream`` (default: torch's current stream); needs no world.
        Returns a TransformedStamp: ``bits`` the destination words on the device, ``dims`` the destination dims and
        ``summary`` a TransformSummary (None with ``summary=False``); reading the summary waits for the call."""
        call = _Call(self, stream)
        dims = _ints(dims)
        o = orientation._c()
        nsrc = region_words(dims)
        ddims = _ints(dims[a] for a in orientation.axis)
        ndst = region_words(ddims) if nsrc else 0
        if nsrc > N.TRANSFORM_MAX_WORDS or ndst > N.TRANSFORM_MAX_WORDS:
            nsrc = ndst = 0  # (one-word placeholders: the library does the refusing)
        src = call.reads(call.fits(bits, nsrc, 4, "bits: a contiguous device tensor of at least region_words(dims) words", any_size=True))
        dst = call.out(ndst, 4, call.torch.int32, out, "out: a contiguous device tensor of at least region_words of the turned dims",
                       any_size=True)
        words = call.summary(8) if summary else None
        call.launch(self._L.vxrt_transform_stamp, _ptr(src), _i3(dims), C.byref(o), _ptr(dst), _ptr(words))
        return TransformedStamp(bits=dst.view(-1)[:ndst] if dst.element_size() == 4 else dst, dims=ddims, orientation=orientation,
                                _summary=words, _stream=call.s)

    def transform_stamp_host(self, grid, orientation: "Orientation", summary: bool = True) -> "TransformedStamp":
        """transform_stamp through the synchronous host call (vxrt_transform_stamp_host): ``grid`` a bool [x, y, z] numpy
        grid, packed and unpacked here; the result's ``bits`` is the turned bool grid."""
        g = np.asarray(grid, bool)
        dims = _ints(g.shape)
        ddims = _ints(dims[a] for a in orientation.axis)
        o = orientation._c()
        src = pack_region(g) if g.size else np.zeros(1, np.uint32)
        dst = np.zeros(max(region_words(ddims), 1), np.uint32)
        words = np.zeros(8, np.uint32) if summary else None
        N.check(self._L.vxrt_transform_stamp_host(self._h, src.ctypes.data, _i3(dims), C.byref(o), dst.ctypes.data,
                                                  words.ctypes.data if summary else None))
        return TransformedStamp(bits=unpack_region(dst, ddims), dims=ddims, orientation=orientation, _summary=words, _stream=None)

    # ---- navigation fields (extension, include/vxrt.h) ----------------------------------------------------------------
    def nav_field(self, origin, dims, goals, agent: "NavAgent | None" = None, max_dist: int = 1 << 24, dist: bool = True,
                  stream: int | None = None) -> "NavField":
        """The navigation field of the box ``origin`` .. ``origin + dims - 1`` for ``agent`` (default NavAgent()) toward the
        world cells ``goals`` (an (n, 3) array, n <= NAV_MAX_GOALS): include/vxrt.h, vxrt_nav_field.  Runs on ``stream``
        (default: torch's current stream) after the work queued there and returns when the field is complete.  Returns a
        NavField of device tensors (walkable region words, one next code per cell, dist when ``dist``) and the summary.

        A body steered with move_boxes can follow ``NavField.paths``: each move is one cell, ``nav_move(code, agent)``."""
        call = _Call(self, stream)
        torch = call.torch
        agent = agent or NavAgent()
        origin, dims = _box(origin, dims)
        g = np.ascontiguousarray(np.asarray(goals, np.int32).reshape(-1, 3))
        ag = agent._c()
        ws = int(self._L.vxrt_nav_workspace_bytes(_i3(dims), C.byref(ag)))
        nvox, nw = _counts(dims, ws)
        work = call.work(ws)
        walk = call.out(nw, 4, torch.int32)
        nxt = call.out(nvox, 1, torch.uint8)
        dst = call.out(nvox, 4, torch.int32) if dist else None
        summary = call.summary(8)
        dg = call.upload(g)
        call.launch(self._L.vxrt_nav_field, _i3(origin), _i3(dims), C.byref(ag), _ptr(dg) if len(g) else None, len(g), int(max_dist),
                    _ptr(work), _ptr(walk), _ptr(nxt), _ptr(dst), _ptr(summary))
        return NavField(origin=origin, dims=dims, agent=agent, walkable=walk[:nw], next=nxt[:nvox], dist=dst[:nvox] if dist else None,
                        summary=NavSummary(*(int(v) for v in summary.cpu().numpy().view(np.uint32))), ctx=self)

    def nav_field_host(self, origin, dims, goals, agent: "NavAgent | None" = None, max_dist: int = 1 << 24) -> "NavField":
        """nav_field through the synchronous host call (vxrt_nav_field_host): numpy outputs -- walkable as a bool [x, y, z]
        grid, next as uint8 [x, y, z], dist as uint32 [x, y, z]."""
        agent = agent or NavAgent()
        origin, dims = _box(origin, dims)
        g = np.ascontiguousarray(np.asarray(goals, np.int32).reshape(-1, 3))
        ag = agent._c()
        nvox, n = _counts(dims, region_words(dims))
        walk = np.zeros(max(n, 1), np.uint32)
        nxt = np.zeros(max(nvox, 1), np.uint8)
        dst = np.zeros(max(nvox, 1), np.uint32)
        summary = np.zeros(8, np.uint32)
        N.check(self._L.vxrt_nav_field_host(self._h, _i3(origin), _i3(dims), C.byref(ag), g.ctypes.data if len(g) else None,
                                            len(g), int(max_dist), walk.ctypes.data, nxt.ctypes.data, dst.ctypes.data,
                                            summary.ctypes.data))
        return NavField(origin=origin, dims=dims, agent=agent, walkable=unpack_region(walk, dims), next=_grid(nxt, dims),
                        dist=_grid(dst, dims), summary=NavSummary(*(int(v) for v in summary)), ctx=self)

    # ---- exact distance fields (extension, include/vxrt.h) -----------------------------------------------------------
    def distance_workspace_bytes(self, dims, radius: int) -> int:
        """vxrt_distance_workspace_bytes: the workspace of one distance_field call, 0 outside the contract"""
        return int(self._L.vxrt_distance_workspace_bytes(_i3(dims), int(radius)))

    def distance_field(self, origin, dims, radius: int, mode: int = N.DIST_TO_SOLID, out=None,
                       stream: int | None = None) -> "DistanceField":
        """The exact squared distance from every voxel of the box ``origin`` .. ``origin + dims - 1`` to the nearest solid
        (``DIST_TO_SOLID``) or empty (``DIST_TO_EMPTY``) voxel of the world within ``radius`` voxels, ``DIST_FAR`` beyond it:
        include/vxrt.h, vxrt_distance_field.  Asynchronous on ``stream`` (default: torch's current stream).  ``out``: a
        device tensor of two-byte elements to write the field to (one per voxel; default: a new one).  Returns a
        DistanceField; reading its ``summary`` waits for the call."""
        call = _Call(self, stream)
        origin, dims = _box(origin, dims)
        ws = self.distance_workspace_bytes(dims, radius)
        nvox, _ = _counts(dims, ws)
        work = call.work(ws)
        out = call.out(nvox, 2, call.torch.int16, out,
                       "out: a contiguous device tensor of at least dims[0] * dims[1] * dims[2] two-byte elements")
        summary = call.summary(6)
        call.launch(self._L.vxrt_distance_field, _i3(origin), _i3(dims), int(radius), int(mode), _ptr(work), _ptr(out), _ptr(summary))
        return DistanceField(origin=origin, dims=dims, radius=int(radius), mode=int(mode), dist2=out.view(-1)[:nvox],
                             _summary=summary, _stream=call.s)

    def distance_field_host(self, origin, dims, radius: int, mode: int = N.DIST_TO_SOLID) -> "DistanceField":
        """distance_field through the synchronous host call (vxrt_distance_field_host): ``dist2`` is a numpy uint16
        [x, y, z] grid."""
        origin, dims = _box(origin, dims)
        nvox, _ = _counts(dims, self.distance_workspace_bytes(dims, radius))
        out = np.zeros(max(nvox, 1), np.uint16)
        summary = np.zeros(6, np.uint32)
        N.check(self._L.vxrt_distance_field_host(self._h, _i3(origin), _i3(dims), int(radius), int(mode), out.ctypes.data,
                                                 summary.ctypes.data))
        return DistanceField(origin=origin, dims=dims, radius=int(radius), mode=int(mode), dist2=_grid(out, dims),
                             _summary=summary, _stream=None)

    # ---- voxel light fields (extension, include/vxrt.h) ------------------------------------------------------------------
    def light_workspace_bytes(self, dims, channels: int = N.LIGHT_SKY | N.LIGHT_BLOCK) -> int:
        """vxrt_light_workspace_bytes: the workspace of one light_field call, 0 outside the contract"""
        c = int(channels)
        return int(self._L.vxrt_light_workspace_bytes(_i3(dims), c)) if 0 <= c < 1 << 32 else 0

    def light_field(self, origin, dims, emitters=None, channels: int = N.LIGHT_SKY | N.LIGHT_BLOCK, out=None, work=None,
                    stream: int | None = None) -> "LightField":
        """The light levels of the box ``origin`` .. ``origin + dims - 1``: include/vxrt.h, vxrt_light_field.  ``emitters``:
        rows of (x, y, z, level) as a numpy array, a list or a device int32 tensor (None: no emitters).  Asynchronous on
        ``stream`` (default: torch's current stream).  ``out``: a device tensor of one-byte elements to write the levels to
        (one per voxel; default: a new one); ``work``: a device tensor of at least light_workspace_bytes bytes to use as
        the workspace (default: a new one).  Returns a LightField; reading its ``summary`` waits for the call."""
        call = _Call(self, stream)
        torch = call.torch
        origin, dims = _box(origin, dims)
        ws = self.light_workspace_bytes(dims, channels)
        nvox, _ = _counts(dims, ws)
        work = call.work(ws, work, "work: a contiguous device tensor of at least light_workspace_bytes(dims, channels) bytes")
        out = call.out(nvox, 1, torch.uint8, out,
                       "out: a contiguous device tensor of at least dims[0] * dims[1] * dims[2] one-byte elements")
        if isinstance(emitters, torch.Tensor):
            em = call.reads(emitters.to(device=call.dev, dtype=torch.int32).contiguous().view(-1, 4))
        else:
            em = call.upload(_emitter_rows(emitters))
        n = em.shape[0]
        summary = call.summary(42)
        call.launch(self._L.vxrt_light_field, _i3(origin), _i3(dims), _ptr(em) if n else None, n, _u32(channels), _ptr(work),
                    _ptr(out), _ptr(summary))
        return LightField(origin=origin, dims=dims, channels=int(channels), levels=out.view(-1)[:nvox], _summary=summary,
                          _stream=call.s)

    def light_field_host(self, origin, dims, emitters=None, channels: int = N.LIGHT_SKY | N.LIGHT_BLOCK) -> "LightField":
        """light_field through the synchronous host call (vxrt_light_field_host): ``levels`` is a numpy uint8 [x, y, z]
        grid."""
        origin, dims = _box(origin, dims)
        nvox, _ = _counts(dims, self.light_workspace_bytes(dims, channels))
        rows = _emitter_rows(emitters)
        out = np.zeros(max(nvox, 1), np.uint8)
        summary = np.zeros(42, np.uint32)
        N.check(self._L.vxrt_light_field_host(self._h, _i3(origin), _i3(dims), rows.ctypes.data if len(rows) else None, len(rows),
                                              _u32(channels), out.ctypes.data, summary.ctypes.data))
        return LightField(origin=origin, dims=dims, channels=int(channels), levels=_grid(out, dims), _summary=summary, _stream=None)

    # ---- voxel rules (extension, include/vxrt.h) ---------------------------------------------------------------------------
    def rule_workspace_bytes(self, dims, rule: "Rule") -> int:
        """vxrt_rule_workspace_bytes: the workspace of one apply_rule call, 0 outside the contract"""
        r = rule._c()
        return int(self._L.vxrt_rule_workspace_bytes(_i3(dims), C.byref(r)))

    def apply_rule(self, origin, dims, rule: "Rule", mask=None, stream: int | None = None, *, out=None, work=None) -> "RuleResult":
        """The voxels of the box ``origin`` .. ``origin + dims - 1`` after ``rule.iterations`` steps of the neighbour-count
        rule: include/vxrt.h, vxrt_apply_rule.  The world is not changed: the result's ``stamp()`` writes it.  ``mask``
        (RULE_BOX only): the voxels a step may change, a bool [x, y, z] numpy grid of ``dims`` or a device tensor of region
        words.  Asynchronous on ``stream`` (default: torch's current stream).  ``out``: a device tensor of at least
        region_words(dims) words for the bits; ``work``: one of at least rule_workspace_bytes bytes (defaults: new ones).
        Returns a RuleResult; reading its ``summary`` waits for the call."""
        call = _Call(self, stream)
        origin, dims = _box(origin, dims)
        r = rule._c()
        ws = self.rule_workspace_bytes(dims, rule)
        _, nw = _counts(dims, ws)
        work = call.work(ws, work, "work: a contiguous device tensor of at least rule_workspace_bytes(dims, rule) bytes")
        bits = call.out(nw, 4, call.torch.int32, out, "out: a contiguous device tensor of at least region_words(dims) words",
                        any_size=True)
        if isinstance(mask, np.ndarray):
            mask = call.upload(_mask_words(mask, dims))
        elif mask is not None:
            mask = call.reads(call.fits(mask, nw, 4, "mask: a contiguous device tensor of at least region_words(dims) words",
                                        any_size=True))
        summary = call.summary(12)
        call.launch(self._L.vxrt_apply_rule, _i3(origin), _i3(dims), C.byref(r), _ptr(mask), _ptr(work), _ptr(bits), _ptr(summary))
        return RuleResult(bits=bits.view(-1)[:nw] if bits.element_size() == 4 else bits, origin=origin, dims=dims, _summary=summary,
                          _stream=call.s)

    def apply_rule_host(self, origin, dims, rule: "Rule", mask=None) -> "RuleResult":
        """apply_rule through the synchronous host call (vxrt_apply_rule_host): ``bits`` is a numpy bool [x, y, z] grid;
        ``mask`` a bool [x, y, z] numpy grid or None."""
        origin, dims = _box(origin, dims)
        r = rule._c()
        _, nw = _counts(dims, self.rule_workspace_bytes(dims, rule))
        words = np.zeros(max(nw, 1), np.uint32)
        summary = np.zeros(12, np.uint32)
        m = None if mask is None else _mask_words(mask, dims)
        N.check(self._L.vxrt_apply_rule_host(self._h, _i3(origin), _i3(dims), C.byref(r), None if m is None else m.ctypes.data,
                                             words.ctypes.data, summary.ctypes.data))
        return RuleResult(bits=unpack_region(words, dims), origin=origin, dims=dims, _summary=summary, _stream=None)

    def smooth_voxels(self, origin, dims, iterations: int = 1, mask=None):
        """apply_rule with Rule.smooth(iterations) on the box alone (RULE_BOX), then one STAMP_REPLACE edit_stamps of its
        result at ``origin``: the box is smoothed in the resident world.  Returns (EditStats, RuleSummary)."""
        res = self.apply_rule(origin, dims, Rule.smooth(iterations), mask)
        st = self.edit_stamps([res.stamp()])
        return st, res.summary

    # ---- loose voxels (extension, include/vxrt.h) -----------------------------------------------------------------------------
    def loose_workspace_bytes(self, dims) -> int:
        """vxrt_loose_workspace_bytes: the workspace of one loose_step call, 0 outside the contract"""
        return int(self._L.vxrt_loose_workspace_bytes(_i3(dims)))

    def loose_step(self, origin, dims, loose, params: "Loose | None" = None, stream: int | None = None, *, out=None,
                   work=None) -> "LooseResult":
        """The loose layer ``loose`` of the box ``origin`` .. ``origin + dims - 1`` after ``params.steps`` steps of falling,
        sliding and (water) spreading over the world's solids: include/vxrt.h, vxrt_loose_step.  The world is not changed.
        ``loose``: a bool [x, y, z] numpy grid of ``dims`` or a device tensor of region words.  Asynchronous on ``stream``
        (default: torch's current stream).  ``out``: a device tensor of at least region_words(dims) words for the new layer --
        it may be ``loose`` itself (a call in place); ``work``: one of at least loose_workspace_bytes bytes (defaults: new
        ones).  Returns a LooseResult; reading its ``summary`` waits for the call."""
        call = _Call(self, stream)
        origin, dims = _box(origin, dims)
        p = (params or Loose())._c()
        ws = self.loose_workspace_bytes(dims)
        _, nw = _counts(dims, ws)
        what = "a contiguous device tensor of at least region_words(dims) words"
        work = call.work(ws, work, "work: a contiguous device tensor of at least loose_workspace_bytes(dims) bytes")
        if isinstance(loose, np.ndarray):
            loose = call.upload(_mask_words(loose, dims))
        else:
            loose = call.reads(call.fits(loose, nw, 4, "loose: " + what, any_size=True))
        bits = call.out(nw, 4, call.torch.int32, out, "out: " + what, any_size=True)
        summary = call.summary(12)
        call.launch(self._L.vxrt_loose_step, _i3(origin), _i3(dims), C.byref(p), _ptr(loose), _ptr(work), _ptr(bits), _ptr(summary))
        return LooseResult(bits=bits.view(-1)[:nw] if bits.element_size() == 4 else bits, origin=origin, dims=dims, _summary=summary,
                           _stream=call.s)

    def loose_step_host(self, origin, dims, loose, params: "Loose | None" = None) -> "LooseResult":
        """loose_step through the synchronous host call (vxrt_loose_step_host): ``loose`` and the result's ``bits`` are bool
        [x, y, z] numpy grids."""
        origin, dims = _box(origin, dims)
        p = (params or Loose())._c()
        _, nw = _counts(dims, self.loose_workspace_bytes(dims))
        words = np.zeros(max(nw, 1), np.uint32)
        summary = np.zeros(12, np.uint32)
        m = _mask_words(loose, dims) if nw else np.zeros(1, np.uint32)
        N.check(self._L.vxrt_loose_step_host(self._h, _i3(origin), _i3(dims), C.byref(p), m.ctypes.data, words.ctypes.data,
                                             summary.ctypes.data))
        return LooseResult(bits=unpack_region(words, dims), origin=origin, dims=dims, _summary=summary, _stream=None)

    def settle_voxels(self, origin, dims, source_origin, source_dims, material: int = N.LOOSE_SAND, max_steps: int = 256,
                      edge: int = N.LOOSE_WALL):
        """Turn the solid voxels of the source box loose and let them settle inside the box ``origin`` .. ``origin + dims -
        1``, which must contain the source box: the source's voxels are lifted out of the world (one STAMP_SUBTRACT), stepped
        in place on the device in calls of at most LOOSE_MAX_STEPS steps with the phase carried, until a call's last step
        neither drops nor slides a voxel or ``max_steps`` steps are made, and stamped back with STAMP_UNION.  Returns
        (LooseSummary of the last call, steps made)."""
        origin, dims = _box(origin, dims)
        so, sd = _box(source_origin, source_dims)
        if int(max_steps) < 1 or material not in (N.LOOSE_SAND, N.LOOSE_WATER) or edge not in (N.LOOSE_WALL, N.LOOSE_OPEN):
            raise ValueError("max_steps: at least 1; material: LOOSE_SAND or LOOSE_WATER; edge: LOOSE_WALL or LOOSE_OPEN")
        if any(a < o or a + b > o + d for a, b, o, d in zip(so, sd, origin, dims)):
            raise ValueError("the source box must lie inside the box")
        before = self.read_region(origin, dims)
        self.edit_stamps([Stamp(so, self.read_region(so, sd), N.STAMP_SUBTRACT, sd)])
        layer = before & ~self.read_region(origin, dims)  # the voxels the stamp took out, in the box's layout
        import torch
        work = torch.empty(max(self.loose_workspace_bytes(dims), 4), dtype=torch.uint8, device=layer.device)
        done, res = 0, None
        while done < int(max_steps):
            n = min(N.LOOSE_MAX_STEPS, int(max_steps) - done)
            res = self.loose_step(origin, dims, layer, Loose(material, n, edge, done & 0xFFFFFFFF), out=layer, work=work)
            done += n
            s = res.summary
            if s.fell_last + s.slid_last == 0:
                break
        self.edit_stamps([res.stamp()])
        return res.summary, done

    # ---- mesh voxelization (extension, include/vxrt.h) ----------------------------------------------------------------
    def voxelize_workspace_bytes(self, dims, n_triangles: int) -> int:
        """vxrt_voxelize_workspace_bytes: the workspace of one voxelize_mesh call, 0 outside the contract"""
        n = int(n_triangles)
        return int(self._L.vxrt_voxelize_workspace_bytes(_i3(dims), n)) if 0 <= n < 1 << 32 else 0

    def voxelize_mesh(self, vertices, triangles, dims, modes: int = N.VOX_SURFACE | N.VOX_SOLID, stream: int | None = None,
                      work=None, out=None) -> "VoxelizedMesh":
        """A triangle mesh as region bits of ``dims`` voxels (include/vxrt.h, vxrt_voxelize_mesh): ``vertices`` (n, 3) int32
        in units of 1 / 256 voxel in the region's frame (``quantize_vertices`` makes them from floats), ``triangles``
        (m, 3) vertex indices; numpy arrays or device tensors.  ``modes``: VOX_SURFACE, VOX_SOLID or both.  Asynchronous on
        ``stream`` (default: torch's current stream).  ``work`` / ``out``: device tensors to reuse as the workspace and the
        output words.  Returns a VoxelizedMesh; ``.bits`` is a stamp's device words as it is."""
        call = _Call(self, stream)
        torch = call.torch
        dims = _ints(dims)

        def on_device(a, np_dtype):
            if isinstance(a, torch.Tensor):
                if a.dtype not in (torch.int32, torch.uint32) or not a.is_contiguous() or a.numel() % 3 or not a.is_cuda:
                    raise ValueError("mesh tensors: contiguous device tensors of int32, 3 per row")
                return call.reads(a)
            return call.upload(_mesh_array(a, np_dtype))

        v, t = on_device(vertices, np.int32), on_device(triangles, np.uint32)
        nv, nt = v.numel() // 3, t.numel() // 3
        ws = self.voxelize_workspace_bytes(dims, nt)
        _, nw = _counts(dims, ws)
        work = call.work(ws, work, "work: a contiguous device tensor of at least voxelize_workspace_bytes(dims, n_triangles) bytes")
        out = call.out(nw, 4, torch.int32, out, "out: a contiguous device tensor of at least region_words(dims) words", any_size=True)
        summary = call.summary(8)
        call.launch(self._L.vxrt_voxelize_mesh, _ptr(v) if nt else None, nv, _ptr(t) if nt else None, nt, _i3(dims), int(modes),
                    _ptr(work), _ptr(out), _ptr(summary))
        return VoxelizedMesh(dims=dims, modes=int(modes), bits=out.view(-1)[:nw] if out.element_size() == 4 else out,
                             _summary=summary, _stream=call.s)

    def voxelize_mesh_host(self, vertices, triangles, dims, modes: int = N.VOX_SURFACE | N.VOX_SOLID) -> "VoxelizedMesh":
        """voxelize_mesh through the synchronous host call (vxrt_voxelize_mesh_host): ``bits`` is a bool [x, y, z] grid."""
        dims = _ints(dims)
        v, t = _mesh_array(vertices, np.int32), _mesh_array(triangles, np.uint32)
        _, nw = _counts(dims, self.voxelize_workspace_bytes(dims, len(t)))
        words = np.zeros(max(nw, 1), np.uint32)
        summary = np.zeros(8, np.uint32)
        N.check(self._L.vxrt_voxelize_mesh_host(self._h, v.ctypes.data if len(t) else None, len(v), t.ctypes.data if len(t) else None,
                                                len(t), _i3(dims), int(modes), words.ctypes.data, summary.ctypes.data))
        return VoxelizedMesh(dims=dims, modes=int(modes), bits=unpack_region(words, dims), _summary=summary, _stream=None)

    def stamp_mesh(self, vertices, triangles, origin, modes: int = N.VOX_SURFACE | N.VOX_SOLID, stamp_mode: int = N.STAMP_UNION):
        """Voxelize a mesh given in WORLD units of 1 / 256 voxel into its own bounding box and write it into the resident
        world with one stamp: the box is the voxels the mesh's bounding box touches, moved by ``origin`` (world voxels).
        Returns (VoxelizedMesh, EditStats, the stamp's origin)."""
        v = np.asarray(vertices).reshape(-1, 3).astype(np.int64)
        t = np.asarray(triangles).reshape(-1, 3)
        used = v[t[t.max(axis=1) < len(v)].reshape(-1)] if len(t) else v[:0]
        if not len(used):
            raise ValueError("stamp_mesh: no triangle with valid indices")
        lo = (used.min(axis=0) - 1) >> 8  # the voxel cubes the bounding box touches
        hi = used.max(axis=0) >> 8
        dims = tuple(int(x) for x in hi - lo + 1)
        m = self.voxelize_mesh((v - 256 * lo).astype(np.int32), t, dims, modes)
        at = tuple(int(a) + int(b) for a, b in zip(origin, lo))
        st = self.edit_stamps([Stamp(at, m.bits, stamp_mode, dims)])
        return m, st, at

    # ---- surface extraction (extension, include/vxrt.h) ---------------------------------------------------------------
    def surface_workspace_bytes(self, dims) -> int:
        """vxrt_surface_workspace_bytes: the workspace of one extract_surface call, 0 outside the contract"""
        return int(self._L.vxrt_surface_workspace_bytes(_i3(dims)))

    def extract_surface(self, origin, dims, mode: int = N.SURF_CAP, triangles: bool = False, capacity: int | None = None,
                        stream: int | None = None) -> "ExtractedSurface":
        """The surface of the box ``origin`` .. ``origin + dims - 1`` of the resident world as merged quads in canonical
        order (include/vxrt.h, vxrt_extract_surface), with ``triangles`` also as vertices and triangles in voxelize_mesh's
        input format.  ``mode``: SURF_CAP (neighbours outside the box are empty: a closed surface) or SURF_OPEN (they are the
        world's voxels).  ``capacity``: quads to make room for; None counts first (one more call, and a wait for it) and
        makes room for all.  Asynchronous on ``stream`` (default: torch's current stream).  Returns an ExtractedSurface of
        device tensors sized to the capacity; its ``summary`` tells how many records were written."""
        call = _Call(self, stream)
        torch = call.torch
        origin, dims = _box(origin, dims)
        work = call.work(self.surface_workspace_bytes(dims))

        def extract(cap, quads, verts, tris):
            summary = call.summary(16)
            call.launch(self._L.vxrt_extract_surface, _i3(origin), _i3(dims), int(mode), _ptr(work), _ptr(quads), cap, _ptr(verts),
                        _ptr(tris), _ptr(summary))
            return summary

        if capacity is None:
            counted = extract(0, None, None, None)
            call.stream.synchronize()
            capacity = int(counted.cpu().numpy().view(np.uint32)[2])
        capacity = int(capacity)
        if not 0 <= capacity < 1 << 32:
            raise ValueError("capacity: 0 .. 2^32 - 1 quads")
        quads = torch.empty((capacity, 2), dtype=torch.int32, device=call.dev)
        verts = torch.empty((4 * capacity, 3), dtype=torch.int32, device=call.dev) if triangles else None
        tris = torch.empty((2 * capacity, 3), dtype=torch.int32, device=call.dev) if triangles else None
        summary = extract(capacity, quads if capacity else None, verts, tris)
        return ExtractedSurface(origin=origin, dims=dims, mode=int(mode), quads=quads, vertices=verts, triangles=tris,
                                _summary=summary, _stream=call.s)

    def extract_surface_host(self, origin, dims, mode: int = N.SURF_CAP, triangles: bool = False,
                             capacity: int | None = None) -> "ExtractedSurface":
        """extract_surface through the synchronous host call (vxrt_extract_surface_host): numpy arrays, cut to the records
        written."""
        origin, dims = _box(origin, dims)

        def call(cap, quads, verts, tris):
            summary = np.zeros(16, np.uint32)
            N.check(self._L.vxrt_extract_surface_host(self._h, _i3(origin), _i3(dims), int(mode), quads.ctypes.data if cap else None,
                                                      cap, verts.ctypes.data if triangles and quads is not None else None,
                                                      tris.ctypes.data if triangles and quads is not None else None,
                                                      summary.ctypes.data))
            return summary

        if capacity is None:
            capacity = int(call(0, None, None, None)[2])
        capacity = int(capacity)
        quads = np.zeros((capacity, 2), np.uint32)
        verts = np.zeros((4 * capacity, 3), np.int32)
        tris = np.zeros((2 * capacity, 3), np.uint32)
        summary = call(capacity, quads, verts, tris)
        n = int(summary[3])
        return ExtractedSurface(origin=origin, dims=dims, mode=int(mode), quads=quads[:n],
                                vertices=verts[:4 * n] if triangles else None, triangles=tris[:2 * n] if triangles else None,
                                _summary=summary, _stream=None)

    # ---- frame denoiser (extension, include/vxrt.h) ---------------------------------------------------------------------
    def frame_guides(self, width: int, height: int, origin, fwd, up, right, hit_aov, ortho: bool = False, out=None,
                     stream: int | None = None):
        """The guide keys of a whole frame (include/vxrt.h, vxrt_frame_guides): per pixel 0 for a miss, else the voxel face the
        pixel's primary ray enters, from ``hit_aov`` (the int64 hit-index AOV of a render of the same size, camera and
        ``ortho`` flag) and the context's FOV / ortho window.  Asynchronous on ``stream`` (default: torch's current stream).
        ``out``: a contiguous device tensor of width * height four-byte elements (default: a new int32 one).  Returns it,
        shaped (height, width)."""
        call = _Call(self, stream)
        width, height = int(width), int(height)
        n = width * height if self.denoise_workspace_bytes(width, height) else 0
        call.reads(call.fits(hit_aov, n, 8, "hit_aov: a contiguous device tensor of width * height int64 elements"))
        out = call.out(n, 4, call.torch.int32, out, "out: a contiguous device tensor of width * height four-byte elements")
        call.launch(self._L.vxrt_frame_guides, _u32(width), _u32(height), _f3(origin), _f3(fwd), _f3(up), _f3(right),
                    1 if ortho else 0, _ptr(hit_aov), _ptr(out))
        return out.view(-1)[:n].view(height, width) if n else out

    def denoise_workspace_bytes(self, width: int, height: int) -> int:
        """vxrt_denoise_workspace_bytes: the workspace of one denoise call (2 * W * H * 16), 0 outside the contract"""
        width, height = int(width), int(height)
        return int(self._L.vxrt_denoise_workspace_bytes(width, height)) if 0 <= width < 1 << 32 and 0 <= height < 1 << 32 else 0

    def denoise_frame(self, color, keys, iterations: int = 4, color_scale: float = 0.0, out=None, fb=None, work=None,
                      stream: int | None = None):
        """The edge-avoiding a-trous filter of include/vxrt.h (vxrt_denoise_frame) over ``color``, a float32 device tensor
        (height, width, 3) such as the colour AOV of a render, guided by ``keys`` (frame_guides): ``iterations`` passes of
        step 1, 2, 4, ..., pixels of one voxel face averaged with B3-spline weights, with ``color_scale`` > 0 also stopped
        by colour distance.  Asynchronous on ``stream`` (default: torch's current stream); the tensors this method allocates
        are torch's, made on torch's current stream, so a ``stream`` other than that one must already be ordered after it.
        ``out``: float32 (height, width, 3), may be ``color`` itself (default: a new tensor); ``fb``: optional uint8
        (height, width, 4) BGRA8 frame written as well; ``work``: a device tensor of at least
        denoise_workspace_bytes(width, height) bytes (default: a new one).  Returns ``out``."""
        call = _Call(self, stream)
        width, height, n = call.frame_inputs(color, keys)
        out = call.frame_outputs(color, n, out, fb)
        work = call.work(self.denoise_workspace_bytes(width, height), work,
                         "work: a contiguous device tensor of at least denoise_workspace_bytes(width, height) bytes", least=16)
        p = N.DenoiseParams(struct_size=C.sizeof(N.DenoiseParams), iterations=int(iterations), color_scale=float(color_scale))
        call.launch(self._L.vxrt_denoise_frame, _u32(width), _u32(height), _ptr(color), _ptr(keys), C.byref(p), _ptr(work), _ptr(out),
                    _ptr(fb))
        return out

    # ---- temporal filter (extension, include/vxrt.h) --------------------------------------------------------------------
    def reproject_frame(self, color, keys, cur, prev, history=None, prev_keys=None, max_history: int = 32, ortho: bool = False,
                        out_history=None, out=None, fb=None, summary: bool = True, stream: int | None = None):
        """The frame history reprojected across a camera move (include/vxrt.h, vxrt_reproject_frame): ``color`` a float32
        device tensor (height, width, 3) such as the colour AOV of a render, ``keys`` its guide keys (frame_guides), ``cur``
        and ``prev`` the cameras of this frame and the previous one as (origin, fwd, up, right), ``history`` and
        ``prev_keys`` the ``history`` and the keys of the previous call's result (either None: no history, every hit pixel
        starts a new mean).  Every hit pixel takes the running mean of the surface point it shows from the previous frame,
        where that frame showed the same voxel face, and blends its colour in: out = m + (c - m) / n, n at most
        ``max_history``.  Asynchronous on ``stream`` (default: torch's current stream), as denoise_frame.
        ``out_history``: float32 (height, width, 4), must not be ``history`` (default: a new tensor); ``out``: float32
        (height, width, 3), may be ``color`` itself (default: a new tensor); ``fb``: optional uint8 (height, width, 4) BGRA8
        frame written as well.  Returns a Reprojected: ``history``, ``color`` and, with ``summary``, a lazily read
        ReprojectSummary."""
        call = _Call(self, stream)
        width, height, n = call.frame_inputs(color, keys)
        if history is not None:
            call.reads(call.fits_f32(history, 4 * n, "history: a contiguous float32 device tensor (height, width, 4)"))
        if prev_keys is not None:
            call.reads(call.fits(prev_keys, n, 4, "prev_keys: a contiguous device tensor of width * height four-byte elements"))
        if out_history is None:
            out_history = call.torch.empty((height, width, 4), dtype=call.torch.float32, device=call.dev)
        else:
            call.fits_f32(out_history, 4 * n, "out_history: a contiguous float32 device tensor (height, width, 4)")
        out = call.frame_outputs(color, n, out, fb)
        words = call.summary(4) if summary else None
        p = N.ReprojectParams(struct_size=C.sizeof(N.ReprojectParams), ortho=1 if ortho else 0, max_history=int(max_history))
        _pose(p.cur, cur)
        _pose(p.prev, prev)
        call.launch(self._L.vxrt_reproject_frame, _u32(width), _u32(height), _ptr(color), _ptr(keys), _ptr(history), _ptr(prev_keys),
                    C.byref(p), _ptr(out_history), _ptr(out), _ptr(fb), _ptr(words))
        return Reprojected(dims=(width, height), history=out_history, color=out, _summary=words, _stream=call.s)

    # ---- light on frames (extension, include/vxrt.h) ---------------------------------------------------------------------
    def light_frame(self, color, keys, hit_aov, cam, field=None, flags: int = N.LF_SMOOTH | N.LF_OCCLUSION, outside_level: int = 0xF0,
                    sky_floor: float = 0.25, block_color=(1.0, 0.8, 0.5), ao_curve=(0.4, 0.6, 0.8, 1.0), ortho: bool = False,
                    box=None, out=None, fb=None, terms=False, summary: bool = True, stream: int | None = None):
        """Smooth voxel light and corner occlusion on a frame (include/vxrt.h, vxrt_light_frame): ``color`` a float32 device
        tensor (height, width, 3) such as the colour AOV of a render or the output of denoise_frame, ``keys`` its guide keys
        (frame_guides), ``hit_aov`` the int64 hit-index AOV of the same render, ``cam`` the camera the frame was rendered
        with as (origin, fwd, up, right).  ``field``: the LightField of Context.light_field (its device levels and its box), or
        a device tensor of one byte per voxel of ``box`` = (origin, dims) in region order, or None: every empty cell has
        ``outside_level`` ((sky << 4) | block), as have the empty cells outside the box.  Every hit pixel's colour c
        becomes (c * (sky_floor + (1 - sky_floor) * S) + block_color * Bk) * A with S, Bk the sky and block light 0 .. 1
        interpolated over the four corners of the voxel face it shows and A the corner occlusion from ``ao_curve`` (the
        factor for 0, 1, 2, 3 open neighbours).  Asynchronous on ``stream`` (default: torch's current stream), as
        denoise_frame.  ``out``: float32 (height, width, 3), may be ``color`` itself (default: a new tensor); ``fb``:
        optional uint8 (height, width, 4) BGRA8 frame written as well; ``terms``: True, or a float32 (height, width, 3) tensor to
        write them to: also return (S, Bk, A) per pixel.
        Returns a LitFrame: ``color``, ``terms`` and, with ``summary``, a lazily read LightFrameSummary."""
        call = _Call(self, stream)
        width, height, n = call.frame_inputs(color, keys, hit_aov)
        levels = None
        if isinstance(field, LightField):
            levels, box = field.levels, (field.origin, field.dims)
        elif field is not None:
            levels = field
        if box is None:
            box = ((0, 0, 0), (1, 1, 1))
        origin, dims = _box(*box)
        if levels is not None:
            nvox = max(dims[0], 0) * max(dims[1], 0) * max(dims[2], 0)
            call.reads(call.fits(levels, nvox, 1, "field: a contiguous device tensor of one byte per voxel of the box"))
        out = call.frame_outputs(color, n, out, fb)
        terms_out = call.frame_plane(terms, (height, width, 3), call.torch.float32, "terms: a contiguous float32 device tensor (height, width, 3)")
        words = call.summary(4) if summary else None
        p = N.LightFrameParams(struct_size=C.sizeof(N.LightFrameParams), ortho=1 if ortho else 0, flags=_u32(flags),
                               outside_level=_u32(outside_level), sky_floor=float(sky_floor))
        p.block_color = (C.c_float * 3)(*[float(v) for v in block_color])
        p.ao_curve = (C.c_float * 4)(*[float(v) for v in ao_curve])
        _pose(p.cam, cam)
        p.box_origin, p.box_dims = _i3(origin), _i3(dims)
        call.launch(self._L.vxrt_light_frame, _u32(width), _u32(height), _ptr(color), _ptr(keys), _ptr(hit_aov), _ptr(levels),
                    C.byref(p), _ptr(out), _ptr(fb), _ptr(terms_out), _ptr(words))
        return LitFrame(dims=(width, height), color=out, terms=terms_out, _summary=words, _stream=call.s)

    # ---- sky on frames (extension, include/vxrt.h) -------------------------------------------------------------------------
    def sky_frame(self, color, keys, cam, sky=None, ortho: bool = False, out=None, fb=None, summary: bool = False, stream: int | None = None):
        """A sky behind a frame and distance fog on it (include/vxrt.h, vxrt_sky_frame): ``color`` a float32 device tensor
        (height, width, 3) such as the colour AOV of a render or the output of light_frame, ``keys`` its guide keys
        (frame_guides), ``cam`` the camera the frame was rendered with as (origin, fwd, up, right), ``sky`` a Sky (default:
        Sky(), a daytime sky without clouds).  Every miss pixel takes the sky colour of its primary ray -- gradient, ground,
        sun glow and disc, and with SKY_CLOUDS a layer of value-noise clouds --, every hit pixel is faded towards the sky
        behind it with the distance of the surface it shows.  The last stage of a frame pipeline, after light_frame.  No
        world is needed.  Asynchronous on ``stream`` (default: torch's current stream), as denoise_frame.  ``out``: float32
        (height, width, 3), may be ``color`` itself (default: a new tensor); ``fb``: optional uint8 (height, width, 4) BGRA8
        frame written as well.  ``summary`` (default False: no counting, the cheaper launch): also count the pixels.  Returns a
        SkyFrame: ``color`` and, with ``summary``, a lazily read SkySummary."""
        call = _Call(self, stream)
        width, height, n = call.frame_inputs(color, keys)
        out = call.frame_outputs(color, n, out, fb)
        words = call.summary(6) if summary else None
        p = (Sky() if sky is None else sky)._c(cam, ortho)
        call.launch(self._L.vxrt_sky_frame, _u32(width), _u32(height), _ptr(color), _ptr(keys), C.byref(p), _ptr(out), _ptr(fb), _ptr(words))
        return SkyFrame(dims=(width, height), color=out, _summary=words, _stream=call.s)

    # ---- voxel materials (extension, include/vxrt.h) -------------------------------------------------------------------------
    def _paint(self, call, paint, paint_box):
        """(device bytes or None, box) of a paint argument: a MaterialField (its bytes and its box), a device uint8 tensor or a
        numpy uint8 [x, y, z] grid over ``paint_box`` = (origin, dims), or None"""
        if isinstance(paint, MaterialField):
            paint, paint_box = paint.materials, (paint.origin, paint.dims)
        if paint_box is None:
            paint_box = ((0, 0, 0), (1, 1, 1))
        origin, dims = _box(*paint_box)
        if paint is None:
            return None, (origin, dims)
        if isinstance(paint, np.ndarray):
            if paint.shape != tuple(dims):
                raise ValueError("paint: a uint8 [x, y, z] grid of the paint box's dims")
            host = np.ascontiguousarray(np.asarray(paint, np.uint8).transpose(2, 1, 0)).reshape(-1)  # region order
            return call.upload_bytes(host), (origin, dims)
        nvox = max(dims[0], 0) * max(dims[1], 0) * max(dims[2], 0)
        return call.reads(call.fits(paint, nvox, 1, "paint: a contiguous device tensor of one byte per voxel of the paint box")), (origin, dims)

    def material_field(self, origin, dims, rules: "MaterialRules", paint=None, paint_box=None, out=None,
                       stream: int | None = None) -> "MaterialField":
        """The material bytes of the box ``origin`` .. ``origin + dims - 1`` (include/vxrt.h, vxrt_material_field): 0 for an
        empty voxel, else the paint byte where ``paint`` has one, else the strata rule of ``rules``.  ``paint``: a
        MaterialField, a device uint8 tensor of one byte per voxel of ``paint_box`` = (origin, dims) in region order, a numpy
        uint8 [x, y, z] grid over it, or None.  Asynchronous on ``stream`` (default: torch's current stream).  ``out``: a
        device tensor of one-byte elements to write to (default: a new one).  Returns a MaterialField; reading its
        ``summary`` waits for the call."""
        call = _Call(self, stream)
        origin, dims = _box(origin, dims)
        d_paint, pbox = self._paint(call, paint, paint_box)
        r = rules._c(pbox)
        ok = all(d >= 1 for d in dims) and dims[0] * dims[1] * dims[2] <= 1 << 28
        nvox = dims[0] * dims[1] * dims[2] if ok else 0
        out = call.out(nvox, 1, call.torch.uint8, out,
                       "out: a contiguous device tensor of at least dims[0] * dims[1] * dims[2] one-byte elements")
        summary = call.summary(260)
        call.launch(self._L.vxrt_material_field, _i3(origin), _i3(dims), C.byref(r), _ptr(d_paint), _ptr(out), _ptr(summary))
        return MaterialField(origin=origin, dims=dims, materials=out.view(-1)[:nvox], _summary=summary, _stream=call.s)

    def material_field_host(self, origin, dims, rules: "MaterialRules", paint=None, paint_box=None) -> "MaterialField":
        """material_field through the synchronous host call (vxrt_material_field_host): ``paint`` a numpy uint8 [x, y, z] grid
        over ``paint_box`` or None; ``materials`` is a numpy uint8 [x, y, z] grid."""
        origin, dims = _box(origin, dims)
        pbox = _box(*(paint_box or ((0, 0, 0), (1, 1, 1))))
        host = None
        if paint is not None:
            if tuple(np.shape(paint)) != tuple(pbox[1]):
                raise ValueError("paint: a uint8 [x, y, z] grid of the paint box's dims")
            host = np.ascontiguousarray(np.asarray(paint, np.uint8).transpose(2, 1, 0)).reshape(-1)
        r = rules._c(pbox)
        ok = all(d >= 1 for d in dims) and dims[0] * dims[1] * dims[2] <= 1 << 28
        nvox = dims[0] * dims[1] * dims[2] if ok else 0
        out = np.zeros(max(nvox, 1), np.uint8)
        summary = np.zeros(260, np.uint32)
        N.check(self._L.vxrt_material_field_host(self._h, _i3(origin), _i3(dims), C.byref(r), host.ctypes.data if host is not None else None,
                                                 out.ctypes.data, summary.ctypes.data))
        return MaterialField(origin=origin, dims=dims, materials=_grid(out, dims) if nvox else out[:0], _summary=summary, _stream=None)

    def material_frame(self, color, keys, hit_aov, cam, rules: "MaterialRules", palette: "Palette", paint=None, paint_box=None,
                       ortho: bool = False, out=None, fb=None, material_aov=False, summary: bool = True, stream: int | None = None):
        """Albedo and textures on a frame (include/vxrt.h, vxrt_material_frame): ``color``, ``keys``, ``hit_aov`` and ``cam``
        as Context.light_frame takes them.  Every hit pixel's colour is multiplied with the tint of the material of the voxel
        it shows (``rules``, ``paint`` as in material_field) and with the texel of that material's tile for the face's class
        (top, side, bottom) in ``palette``'s atlas.  In a frame pipeline the stage runs after denoise_frame and before
        light_frame.  Asynchronous on ``stream`` (default: torch's current stream).  ``out``: float32 (height, width, 3), may
        be ``color`` itself (default: a new tensor); ``fb``: optional uint8 (height, width, 4) BGRA8 frame written as well;
        ``material_aov``: True, or a uint8 (height, width) device tensor to write to: also return the material id per pixel.
        Returns a MaterialFrame: ``color``, ``materials`` and, with ``summary``, a lazily read MaterialFrameSummary."""
        call = _Call(self, stream)
        width, height, n = call.frame_inputs(color, keys, hit_aov)
        d_paint, pbox = self._paint(call, paint, paint_box)
        r = rules._c(pbox)
        d_palette, d_atlas = palette._device(call)
        out = call.frame_outputs(color, n, out, fb)
        aov = call.frame_plane(material_aov, (height, width), call.torch.uint8, "material_aov: a contiguous uint8 device tensor (height, width)")
        words = call.summary(4) if summary else None
        p = N.MaterialFrameParams(struct_size=C.sizeof(N.MaterialFrameParams), ortho=1 if ortho else 0, n_tiles=_u32(palette.n_tiles),
                                  tile_shift=_u32(palette.tile_shift))
        _pose(p.cam, cam)
        call.launch(self._L.vxrt_material_frame, _u32(width), _u32(height), _ptr(color), _ptr(keys), _ptr(hit_aov), C.byref(r),
                    _ptr(d_paint), _ptr(d_palette), _ptr(d_atlas), C.byref(p), _ptr(out), _ptr(fb), _ptr(aov), _ptr(words))
        return MaterialFrame(dims=(width, height), color=out, materials=aov, _summary=words, _stream=call.s)

    # ---- occupancy LOD (extension, include/vxrt.h) ----------------------------------------------------------------------
    def lod_workspace_bytes(self, dims, shift: int) -> int:
        """vxrt_lod_workspace_bytes: the workspace of one downsample call, 0 outside the contract"""
        shift = int(shift)
        return int(self._L.vxrt_lod_workspace_bytes(_i3(dims), shift)) if 0 <= shift < 1 << 32 else 0

    def downsample(self, origin, dims, shift: int, threshold: int = 1, counts: bool = False, out=None, work=None,
                   stream: int | None = None) -> "Downsampled":
        """The box of ``dims`` cells of (1 << shift)^3 voxels at world voxel ``origin`` reduced to one bit per cell: set when
        the cell holds at least ``threshold`` solid voxels (1: any, the conservative choice; f^3: all), as region words of
        ``dims`` -- a Stamp's bits for a coarser world -- and with ``counts`` one two-byte count per cell in region order
        (include/vxrt.h, vxrt_downsample_region).  Asynchronous on ``stream`` (default: torch's current stream); the tensors
        this method allocates are torch's, made on torch's current stream, so a ``stream`` other than that one must already be
        ordered after it (as for the other queries).  ``out``: a
        device tensor of region_words(dims) four-byte elements for the bits; ``work``: a device tensor of at least
        lod_workspace_bytes(dims, shift) bytes (default: new ones).  Returns a Downsampled; reading its ``summary`` waits for
        the call."""
        call = _Call(self, stream)
        torch = call.torch
        origin, dims = _box(origin, dims)
        ws = self.lod_workspace_bytes(dims, shift)
        ncell, n = _counts(dims, ws)
        work = call.work(ws, work, "work: a contiguous device tensor of at least lod_workspace_bytes(dims, shift) bytes")
        out = call.out(n, 4, torch.int32, out, "out: a contiguous device tensor of at least region_words(dims) four-byte elements")
        cnt = call.out(ncell, 2, torch.int16) if counts else None
        summary = call.summary(8)
        call.launch(self._L.vxrt_downsample_region, _i3(origin), _i3(dims), _u32(shift), _u32(threshold), _ptr(work), _ptr(out),
                    _ptr(cnt), _ptr(summary))
        return Downsampled(origin=origin, dims=dims, shift=int(shift), threshold=int(threshold), bits=out.view(-1)[:n],
                           counts=cnt[:ncell] if counts else None, _summary=summary, _stream=call.s)

    def downsample_host(self, origin, dims, shift: int, threshold: int = 1, counts: bool = True) -> "Downsampled":
        """downsample through the synchronous host call (vxrt_downsample_region_host): ``bits`` is a numpy bool [x, y, z] grid
        and ``counts`` a numpy uint16 [x, y, z] grid (None without ``counts``)."""
        origin, dims = _box(origin, dims)
        ncell, n = _counts(dims, self.lod_workspace_bytes(dims, shift))
        words = np.zeros(max(n, 1), np.uint32)
        cnt = np.zeros(max(ncell, 1), np.uint16)
        summary = np.zeros(8, np.uint32)
        N.check(self._L.vxrt_downsample_region_host(self._h, _i3(origin), _i3(dims), _u32(shift), _u32(threshold), words.ctypes.data,
                                                    cnt.ctypes.data if counts else None, summary.ctypes.data))
        return Downsampled(origin=origin, dims=dims, shift=int(shift), threshold=int(threshold), bits=unpack_region(words, dims),
                           counts=_grid(cnt, dims) if counts else None, _summary=summary, _stream=None)

    def lod_world(self, shift: int, threshold: int = 1, into: "Context | None" = None, box=None,
                  slab_cells: int | None = None) -> "Context":
        """A coarser copy of the resident world in a Context of its own: voxel C of it is the bit of cell C of
        ``downsample((0, 0, 0), ..., shift, threshold)``, so it is rendered by the unchanged tracer with the camera scaled by
        1 / f, f = 1 << shift.

        ``into=None`` opens a second Context on this device, uploads an empty world of ceil(world / f) voxels per axis
        (rounded up to whole bricks and to 8 bricks per axis, the shape rule of upload_world) with the same brick factor and
        fills it.  ``into`` with ``box = (lo, hi)``, a box of world voxels with inclusive corners such as an edit's bounding
        box, refreshes an existing LOD world of this shift: the box grows outwards to multiples of f and only those cells are
        written again (``box=None``: all of them).  ``into`` must have the brick factor and the size that ``into=None`` gives for
        this shift, and a world that lod_world made must have been made at this shift (ValueError otherwise): a world of
        another shift would be stamped in the wrong places.

        The cells are filled in z slabs of ``slab_cells`` cells (default: as many as the 2^32-voxel source limit of one
        downsample allows), each one downsample followed by one STAMP_REPLACE stamp into the LOD world; the bits never leave
        the device.  The stamp's cost rules and its synchronisation are vxrt_edit_stamps' own: each stamp synchronises the
        device before and after, and costs in proportion to the LOD bricks its box touches.  Returns the LOD Context."""
        shift, f = int(shift), 1 << int(shift)
        if not 1 <= shift <= N.LOD_MAX_SHIFT:
            raise ValueError("shift: 1 .. LOD_MAX_SHIFT")
        info = self.world_info()
        F = int(info.factor)
        cells = [-(-int(c) * F // f) for c in info.cdims]  # cells that meet the world, per axis
        if into is None:
            if box is not None:
                raise ValueError("box refreshes an existing LOD world: give into")
            cd = [max(-(-(-(-n // F)) // 8) * 8, 8) for n in cells]
            ncells = cd[0] * cd[1] * cd[2]
            into = Context(self.device)
            try:
                into.upload_world(F, cd, np.zeros((ncells + 31) // 32, np.uint32), np.full(ncells, N.EMPTY_SLOT, np.uint32),
                                  np.zeros(6 * ncells, np.float32), np.zeros(0, np.uint32))
                into._lod_shift = shift  # a later refresh at another shift is refused
                return self._lod_fill(into, shift, threshold, cells, None, slab_cells)
            except BaseException:
                into.close()  # the context opened here does not outlive a failure
                raise
        have = into.world_info()
        if int(have.factor) != F or [int(c) for c in have.cdims] != [max(-(-(-(-n // F)) // 8) * 8, 8) for n in cells]:
            raise ValueError("into: not an LOD world of this world at this shift (brick factor or size differ)")
        if getattr(into, "_lod_shift", shift) != shift:
            raise ValueError("into: an LOD world of shift %d, not %d" % (into._lod_shift, shift))
        return self._lod_fill(into, shift, threshold, cells, box, slab_cells)

    def _lod_fill(self, into: "Context", shift: int, threshold: int, cells, box, slab_cells) -> "Context":
        """lod_world's slabs: the cells of ``box`` (all of ``cells`` when None) downsampled and stamped into ``into``"""
        import torch
        f = 1 << shift
        lo, hi = [0, 0, 0], list(cells)  # the cell box [lo, hi)
        if box is not None:
            lo = [max(int(a) // f, 0) for a in box[0]]
            hi = [min(int(b) // f + 1, n) for b, n in zip(box[1], cells)]
        d = [b - a for a, b in zip(lo, hi)]
        if min(d) < 1:
            return into
        per_slab = f ** 3 * d[0] * d[1]
        if per_slab > 1 << 32:
            raise ValueError("one z slab of the cell box exceeds the 2^32-voxel source limit of a downsample")
        most = (1 << 32) // per_slab
        slab = most if slab_cells is None else int(slab_cells)
        if not 1 <= slab <= most:
            raise ValueError("slab_cells: 1 .. %d for this box and shift" % most)
        slab = min(slab, d[2])
        dev = "cuda:%d" % self.device
        work = torch.empty(max(self.lod_workspace_bytes((d[0], d[1], slab), shift), 4), dtype=torch.uint8, device=dev)
        bits = torch.empty(region_words((d[0], d[1], slab)), dtype=torch.int32, device=dev)
        for z in range(lo[2], hi[2], slab):
            dz = (d[0], d[1], min(slab, hi[2] - z))
            got = self.downsample((lo[0] * f, lo[1] * f, z * f), dz, shift, threshold, out=bits, work=work)
            into.edit_stamps([Stamp((lo[0], lo[1], z), got.bits, N.STAMP_REPLACE, dz)])
        return into

    def download_world(self, with_pool: bool = True):
        info = self.world_info()
        n = int(info.ncells)
        cb = np.empty((n + 31) // 32, np.uint32)
        bs = np.empty(n, np.uint32)
        bd = np.empty((n, 6), np.float32)
        bw = info.factor ** 3 // 32
        pl = np.empty(int(info.nslots) * bw, np.uint32) if with_pool else None
        N.check(self._L.vxrt_download_world(self._h, cb.ctypes.data, bs.ctypes.data, bd.ctypes.data,
                                            pl.ctypes.data if (with_pool and pl.size) else None))
        return dict(factor=int(info.factor), cdims=tuple(info.cdims), coarse_bits=cb, brick_slot=bs, bounds=bd,
                    pool=pl)

    # ---- state ----------------------------------------------------------------------------------
    def SetEnvironment(self, light_dir, light_color, ambient) -> None:
        N.check(self._L.vxrt_set_environment(self._h, _f3(light_dir), _f3(light_color), _f3(ambient)))

    def SetFOV(self, fov: float) -> None:
        N.check(self._L.vxrt_set_fov(self._h, float(fov)))

    def SetOrthoWindowSize(self, sx: float, sy: float) -> None:
        N.check(self._L.vxrt_set_ortho_window_size(self._h, float(sx), float(sy)))

    # ---- per frame -------------------------------------------------------------------------------
    def RenderScreen(self, width: int, height: int, d_fb, origin, fwd, up, right, opts: RenderOptions | None = None,
                     color_aov=None, hit_aov=None, stream: int | None = None, tile_order=None, accum=None,
                     accum_reset: bool = False) -> None:
        """Graphics::RenderScreen (VoxelRT/Renderer.cu:305-328).  ``d_fb``/AOVs: torch CUDA tensors or raw
        device addresses.  Asynchronous on ``stream`` (default: torch's current stream)."""
        fl = self._flags(opts, stream)
        fl.d_color_aov = _ptr(color_aov)
        fl.d_hit_aov = _ptr(hit_aov)
        fl.d_tile_order = _ptr(tile_order)
        fl.d_accum = _ptr(accum)  # temporal accumulation history, (H, W, 4) float32 (extension, include/vxrt.h)
        fl.accum_reset = int(bool(accum_reset))
        N.check(self._L.vxrt_render(self._h, width, height, _ptr(d_fb), _f3(origin), _f3(fwd), _f3(up), _f3(right),
                                    C.byref(fl)))

    def _flags(self, opts: RenderOptions | None, stream: int | None) -> "N.RenderFlags":
        o = opts or RenderOptions()
        fl = N.RenderFlags()
        self._L.vxrt_render_flags_default(C.byref(fl))
        fl.mode, fl.checkerboard, fl.shadow = int(o.mode), int(o.checkerboard), int(o.shadow)
        fl.bounce_samples, fl.bounce_all_hits, fl.ortho = int(o.bounce_samples), int(o.bounce_all_hits), int(o.ortho)
        fl.frame_number = int(o.frame_number)
        fl.strip_rows, fl.strip_count, fl.strip_index = int(o.strip_rows), int(o.strip_count), int(o.strip_index)
        fl.compact, fl.collect_stats = int(o.compact), int(o.collect_stats)
        fl.tile_schedule = int(o.tile_schedule)
        fl.bounce_depth = int(o.bounce_depth)
        fl.stream = _stream(stream)
        return fl

    def RenderViews(self, width: int, height: int, views, opts: RenderOptions | None = None,
                    stream: int | None = None) -> None:
        """Several views of the resident world in ONE launch (vxrt_render_views): the next view's first tiles fill
        the lanes the previous view's last rays leave.  ``views``: sequence of dicts with keys ``fb, origin, fwd, up,
        right`` and optionally ``frame_number`` (default: ``opts.frame_number``, or the context counter), ``color_aov``,
        ``hit_aov``.  Every view equals what :meth:`RenderScreen` produces for it."""
        fl = self._flags(opts, stream)
        if opts is not None and opts.extra.get("accum") is not None:
            fl.d_accum = _ptr(opts.extra["accum"])  # rejected by the library: a multi-view launch has no per-view history
        arr = (N.View * len(views))()
        for dst, v in zip(arr, views):
            dst.d_fb = _ptr(v["fb"])
            dst.origin, dst.fwd, dst.up, dst.right = _f3(v["origin"]), _f3(v["fwd"]), _f3(v["up"]), _f3(v["right"])
            dst.frame_number = int(v.get("frame_number", fl.frame_number))
            dst.d_color_aov = _ptr(v.get("color_aov"))
            dst.d_hit_aov = _ptr(v.get("hit_aov"))
        N.check(self._L.vxrt_render_views(self._h, width, height, len(views), arr, C.byref(fl)))

    def frame_stats(self) -> "N.FrameStats":
        st = N.FrameStats()
        N.check(self._L.vxrt_frame_stats_get(self._h, C.byref(st)))
        return st

    def loop_counters(self) -> dict:
        """The loop diagnostics the last frame_stats() read that FrameStats has no field for (vxrt_loop_counters_get)."""
        names = ("co_runs", "co_starts", "end_bounce")
        out = (C.c_uint64 * len(names))()
        n = self._L.vxrt_loop_counters_get(self._h, out, len(names))
        if n < 0:
            N.check(n)
        assert n == len(names), "vxrt_loop_counters_get reports %d counters" % n
        return {k: int(out[i]) for i, k in enumerate(names)}

    def deinterleave_strips(self, width, height, strip_rows, strip_count, d_shards, shard_stride_bytes, d_fb,
                            stream: int | None = None) -> None:
        N.check(self._L.vxrt_deinterleave_strips(self._h, width, height, strip_rows, strip_count, _ptr(d_shards),
                                                 int(shard_stride_bytes), _ptr(d_fb), _stream(stream)))

    def deinterleave_views(self, width, height, strip_rows, strip_count, d_shards, shard_stride_bytes, view_stride_bytes,
                           n_views, d_fb, fb_stride_bytes, stream: int | None = None) -> None:
        """The strips of all `n_views` views of one multi-view step in one launch (vxrt_deinterleave_views)."""
        N.check(self._L.vxrt_deinterleave_views(self._h, width, height, strip_rows, strip_count, _ptr(d_shards),
                                                int(shard_stride_bytes), int(view_stride_bytes), int(n_views), _ptr(d_fb),
                                                int(fb_stride_bytes), _stream(stream)))

    # ---- batch -----------------------------------------------------------------------------------
    def set_batch_max_steps(self, max_steps: int) -> None:
        """``maxSteps`` of the device function ``Raytrace`` for the following batch calls (default 2048; the
        reference's secondary rays use 8, VoxelRT/Renderer.cu:141)."""
        N.check(self._L.vxrt_set_batch_max_steps(self._h, int(max_steps)))

    def Raytrace(self, origins, dirs, want_stats: bool = False):
        """VoxelRaytracer3D::Raytrace (VoxelRT/VolumeRaytracer.cu:574-618) on host arrays: copy in, trace,
        copy out.  Returns the reference's fields (hitPoint=+inf on a miss, normal, steps, valid, distance)
        plus this build's hit voxel index."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = o.shape[0]
        pos = np.empty((n, 3), np.float32)
        nrm = np.empty((n, 3), np.float32)
        steps = np.empty(n, np.int32)
        hit = np.empty(n, np.uint8)
        vox = np.empty(n, np.int64)
        st = N.FrameStats()
        N.check(self._L.vxrt_trace_batch_host(self._h, o.ctypes.data, d.ctypes.data, n, pos.ctypes.data,
                                              nrm.ctypes.data, steps.ctypes.data, hit.ctypes.data, vox.ctypes.data,
                                              C.byref(st) if want_stats else None))
        valid = np.isfinite(pos).all(axis=1)
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(((o - pos) ** 2).sum(axis=1, dtype=np.float32))
        return dict(hitPoint=pos, normal=nrm, steps=steps, valid=valid, distance=dist, hit=hit, voxel=vox,
                    stats=st if want_stats else None)

    def trace_batch_device(self, d_origins, d_dirs, n, d_pos, d_normal, d_steps, d_hit=None, d_voxel=None,
                           want_stats=False, stream: int | None = None):
        st = N.FrameStats()
        N.check(self._L.vxrt_trace_batch(self._h, _ptr(d_origins), _ptr(d_dirs), int(n), _ptr(d_pos), _ptr(d_normal),
                                         _ptr(d_steps), _ptr(d_hit), _ptr(d_voxel),
                                         C.byref(st) if want_stats else None, _stream(stream)))
        return st if want_stats else None

    def set_kernel_variant(self, variant: int) -> None:
        """7 = the product kernels (persistent wavefronts on the wave-level tracer of csrc/vxrt_wave2.hpp), 4 = the default
        (= 7), 1 = straightforward per-lane loops (cross-check).  kernel_for_launch tells which kernel a launch runs."""
        N.check(self._L.vxrt_set_kernel_variant(self._h, int(variant)))
        self.kernel_variant = int(variant)

    def set_persistent_waves_per_cu(self, waves_per_cu: int) -> None:
        """Grid of the persistent kernels in wavefronts per CU at 4 waves per SIMD (0 = default 16); tests use a small
        grid so that modest batches take the queue kernel."""
        N.check(self._L.vxrt_set_persistent_waves_per_cu(self._h, int(waves_per_cu)))

    def guard_pretend_no_slack(self, on: bool) -> None:
        """Test hook (vxrt_debug_guard_pretend_no_slack): the load guard of collect_stats launches treats the bit tables as
        allocated without slack."""
        N.check(self._L.vxrt_debug_guard_pretend_no_slack(self._h, int(bool(on))))

    def has_experiments(self) -> bool:
        """True for the A/B build of the library (development knobs read from the environment)."""
        return bool(self._L.vxrt_has_experiments())

    KERNEL_NAMES = {1: "k_render", 7: "k_render_persist2"}

    def kernel_for_launch(self, width: int, height: int, opts: "RenderOptions | None" = None, nviews: int = 0) -> int:
        """The kernel (7 or 1) a RenderScreen (nviews = 0) or RenderViews launch of this shape runs under the
        current variant (vxrt_kernel_for_launch); KERNEL_NAMES maps it to the kernel's name in a profile."""
        fl = self._flags(opts, None)
        k = int(self._L.vxrt_kernel_for_launch(self._h, int(width), int(height), C.byref(fl), int(nviews)))
        if k < 0:
            raise N.VxrtError("vxrt_kernel_for_launch: bad arguments")
        return k

    def render_specialisation(self, width: int, height: int, opts: "RenderOptions | None" = None, nviews: int = 0,
                              hit_aov=None, accum=None) -> int:
        """1 when a RenderScreen (nviews = 0) or RenderViews launch of this shape runs the persistent kernel's
        instantiation for plain shaded frames on brick edge 32 (vxrt_render_specialisation), 0 when it runs the general
        one.  ``hit_aov`` / ``accum``: what the launch would pass (for RenderViews: any view's hit-index AOV).  Host only."""
        fl = self._flags(opts, None)
        fl.d_hit_aov = _ptr(hit_aov)
        fl.d_accum = _ptr(accum)
        k = int(self._L.vxrt_render_specialisation(self._h, int(width), int(height), C.byref(fl), int(nviews)))
        if k < 0:
            raise N.VxrtError("vxrt_render_specialisation: bad arguments")
        return k

    def synchronize(self) -> None:
        N.check(self._L.vxrt_synchronize(self._h))


def _edit_op(kind: int, value: int, a, b) -> "N.EditOp":
    op = N.EditOp()
    op.kind, op.value = int(kind), int(value)
    op.a = (C.c_int32 * 3)(*[int(v) for v in a])
    op.b = (C.c_int32 * 3)(*[int(v) for v in b])
    return op


def EditBox(lo, hi, value: int = 1) -> "N.EditOp":
    """Every voxel v with lo <= v <= hi on each axis (inclusive) set (value 1) or cleared (value 0)."""
    return _edit_op(N.EDIT_BOX, value, lo, hi)


def EditSphere(centre, radius: int, value: int = 1) -> "N.EditOp":
    """Every voxel v with |v - centre|^2 <= radius^2 (integers) set (value 1) or cleared (value 0)."""
    return _edit_op(N.EDIT_SPHERE, value, centre, (radius, 0, 0))


@dataclass
class Stamp:
    """A voxel stamp (include/vxrt.h, vxrt_stamp): ``bits`` a bool [x, y, z] numpy grid, or a device tensor of region
    words with ``dims`` given; ``mode`` STAMP_REPLACE (0), STAMP_UNION (1) or STAMP_SUBTRACT (2)."""
    origin: tuple
    bits: object
    mode: int = N.STAMP_REPLACE
    dims: tuple | None = None


@dataclass
class Body:
    """An axis-aligned box of world voxel coordinates (include/vxrt.h, vxrt_body) and the displacement a move_boxes call
    applies to it; ``Body.pack`` makes the (n, 9) float32 rows the queries take."""
    lo: tuple
    hi: tuple
    delta: tuple = (0.0, 0.0, 0.0)

    def row(self) -> np.ndarray:
        return np.asarray([*self.lo, *self.hi, *self.delta], np.float32)

    @staticmethod
    def pack(bodies) -> np.ndarray:
        return np.stack([b.row() for b in bodies]) if len(bodies) else np.zeros((0, 9), np.float32)


@dataclass
class Piece:
    """A rigid voxel piece (include/vxrt.h, vxrt_piece): ``bits`` a bool [x, y, z] numpy grid (packed on the host as
    edit_stamps packs a stamp), or region words (a device tensor, or a uint32 numpy array) with ``dims`` given."""
    bits: object
    dims: tuple | None = None


class Placement(NamedTuple):
    """vxrt_placement: piece index, the world voxel of the piece's voxel (0, 0, 0), the sweep's axis and signed distance"""
    piece: int
    origin: tuple
    axis: int = 1
    dist: int = 0


PLACED_DTYPE = np.dtype([("overlap", "<u4"), ("travel", "<i4"), ("contact", "<u4"), ("flags", "<u4")])  # vxrt_placed
DROP_DTYPE = np.dtype([("id", "<u4"), ("voxels", "<u4"), ("travel", "<i4"), ("contact", "<u4")])  # drop_islands rows


def _placements_np(placements) -> np.ndarray:
    if isinstance(placements, (list, tuple)):
        placements = [[p.piece, *p.origin, p.axis, p.dist] if isinstance(p, Placement) else list(p) for p in placements]
    pl = np.ascontiguousarray(np.asarray(placements, np.int64).reshape(-1, 6).astype(np.int32))
    return pl


ISLAND_DTYPE = np.dtype([("id", "<u4"), ("voxels", "<u4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,))])  # vxrt_island


class IslandSummary(NamedTuple):
    """vxrt_island_summary: components of the box, islands among them (the true count), voxels of all islands"""
    components: int
    islands: int
    island_voxels: int


def _island_table(rows) -> np.ndarray:
    return np.ascontiguousarray(rows, np.int32).reshape(-1, 8).view(ISLAND_DTYPE).reshape(-1)


@dataclass
class Islands:
    """The result of Context.find_islands: ``floating`` the island voxels (region words on the device; a bool grid from
    find_islands_host), ``labels`` the component id of every voxel (or None), ``table`` a numpy array of ISLAND_DTYPE rows
    (id, voxels, lo[3], hi[3] in world voxels, hi exclusive) in ascending id, ``summary`` an IslandSummary."""
    origin: tuple
    dims: tuple
    floating: object
    labels: object
    table: np.ndarray
    summary: IslandSummary

    def bodies(self, delta=(0.0, 0.0, 0.0)) -> list:
        """One Body per table row -- the island's box, displaced by ``delta`` -- for move_boxes (falling debris).  A box
        wider than BODY_MAX_EXTENT on some axis is an invalid body there: move_boxes returns it unchanged with BODY_INVALID."""
        return [Body(tuple(float(v) for v in r["lo"]), tuple(float(v) for v in r["hi"]), tuple(delta)) for r in self.table]


def _mesh_array(a, np_dtype) -> np.ndarray:
    """integer vertices (int32) or triangle indices (uint32) as a contiguous (n, 3) array: any integer input whose values fit"""
    a = np.asarray(a)
    if a.size == 0:
        return np.zeros((0, 3), np_dtype)
    if a.dtype.kind not in "iu":
        raise TypeError("mesh arrays hold integers (quantize_vertices makes vertices from floats)")
    if a.size % 3:
        raise ValueError("mesh arrays: 3 values per row")
    info = np.iinfo(np_dtype)
    if int(a.min()) < info.min or int(a.max()) > info.max:
        raise ValueError("mesh array values outside %s" % np.dtype(np_dtype).name)
    return np.ascontiguousarray(a.reshape(-1, 3).astype(np_dtype))


def _emitter_rows(emitters) -> np.ndarray:
    """host emitters (None, a list or a numpy array) as contiguous (n, 4) int32 rows x, y, z, level"""
    return np.ascontiguousarray(np.asarray([] if emitters is None else emitters, np.int32).reshape(-1, 4))


def quantize_vertices(xyz) -> np.ndarray:
    """float voxel coordinates -> the int32 fixed point of voxelize_mesh: x * 256 rounded half to even"""
    return np.rint(np.asarray(xyz, np.float64) * 256.0).astype(np.int32).reshape(-1, 3)


class VoxelizeSummary(NamedTuple):
    """vxrt_voxelize_summary: bits set in the output, in the surface field and in the solid field (0 for a field not chosen);
    the triangles given, and those invalid, degenerate and with a bounding box that misses the region"""
    set: int
    surface: int
    solid: int
    triangles: int
    invalid: int
    degenerate: int
    outside: int


class _LazyResult:
    """What the results of the asynchronous queries share.  Each is a dataclass that ends in ``_summary`` (the summary words:
    a device tensor until first read, then a numpy uint32 array; a numpy array from the start in a host result) and
    ``_stream`` (the raw handle of the call's stream; None in a host result), and has ``dims``."""

    def _host(self, t, np_dtype) -> np.ndarray:
        """a numpy array as it is; a device tensor copied to the host once the call's stream has passed the call"""
        if isinstance(t, np.ndarray):
            return t
        import torch
        torch.cuda.ExternalStream(self._stream, device=t.device).synchronize()
        return t.cpu().numpy().view(np_dtype)

    def _words(self) -> list:
        """the summary words as ints; for a device result the first read waits for the call's stream"""
        self._summary = self._host(self._summary, np.uint32)
        return [int(x) for x in self._summary]

    def _xyz(self, t, np_dtype) -> np.ndarray:
        """one value per voxel as a numpy [x, y, z] grid: a host result holds one already, a device result region order"""
        return t if isinstance(t, np.ndarray) else _grid(self._host(t, np_dtype), self.dims)

    def _bits(self, t) -> np.ndarray:
        """bits as a numpy bool [x, y, z] grid: a host result holds one already, a device result region words"""
        return t if isinstance(t, np.ndarray) else unpack_region(self._host(t, np.uint32), self.dims)


@dataclass
class VoxelizedMesh(_LazyResult):
    """The result of Context.voxelize_mesh: ``bits`` the region words on the device (a bool [x, y, z] grid from
    voxelize_mesh_host), ``summary`` a VoxelizeSummary."""
    dims: tuple
    modes: int
    bits: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> VoxelizeSummary:
        """the summary; for a device result this waits for the call's stream"""
        return VoxelizeSummary(*self._words()[:7])

    def grid(self) -> np.ndarray:
        """the voxels as a bool [x, y, z] numpy grid (device words are copied to the host)"""
        return self._bits(self.bits)


class SurfaceSummary(NamedTuple):
    """vxrt_surface_summary: solid voxels of the box, faces, quads (the full count), quads written, faces and quads by
    direction (-x, +x, -y, +y, -z, +z)"""
    solid: int
    faces: int
    quads: int
    written: int
    faces_dir: tuple
    quads_dir: tuple


@dataclass
class ExtractedSurface(_LazyResult):
    """The result of Context.extract_surface: ``quads`` (capacity, 2) words pos, ext; ``vertices`` (4 * capacity, 3) int32 at
    256 units per voxel in the box's frame and ``triangles`` (2 * capacity, 3) indices, or None; device tensors (numpy arrays
    cut to the records written from extract_surface_host).  Only the first ``summary.written`` quads hold records."""
    origin: tuple
    dims: tuple
    mode: int
    quads: object
    vertices: object
    triangles: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> SurfaceSummary:
        """the summary; for a device result this waits for the call's stream"""
        w = self._words()
        return SurfaceSummary(*w[:4], tuple(w[4:10]), tuple(w[10:16]))

    def decode(self):
        """the written quads as numpy arrays (d, x, y, z, w, h): direction, lowest box-relative voxel, extent along u and v"""
        q = np.ascontiguousarray(self._host(self.quads[: self.summary.written], np.uint32)).view(np.uint32).reshape(-1, 2)
        pos, ext = q[:, 0], q[:, 1]
        return (ext >> 20, pos & 1023, pos >> 10 & 1023, pos >> 20 & 1023, (ext & 1023) + 1, (ext >> 10 & 1023) + 1)


class LodSummary(NamedTuple):
    """vxrt_lod_summary: the solid voxels of the source box (the sum of all counts), the cells at or above the threshold, the
    cells with no solid voxel, with f^3 and with something between, the largest count"""
    solid: int
    set: int
    empty: int
    full: int
    mixed: int
    max_count: int


@dataclass
class Downsampled(_LazyResult):
    """The result of Context.downsample: ``bits`` the cell bits as region words of ``dims`` on the device (a Stamp's bits),
    ``counts`` one two-byte count per cell in region order or None; from downsample_host a numpy bool [x, y, z] grid and a
    numpy uint16 [x, y, z] grid.  ``summary`` is a LodSummary."""
    origin: tuple
    dims: tuple
    shift: int
    threshold: int
    bits: object
    counts: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> LodSummary:
        """the summary; for a device result this waits for the call's stream"""
        w = self._words()
        return LodSummary(w[0] | w[1] << 32, *w[2:7])

    def grid(self) -> np.ndarray:
        """the cell bits as a numpy bool [x, y, z] grid (a device result is copied to the host)"""
        return self._bits(self.bits)

    def count_grid(self) -> np.ndarray:
        """the counts as a numpy uint16 [x, y, z] grid (a device result is copied to the host)"""
        if self.counts is None:
            raise ValueError("the call asked for no counts")
        return self._xyz(self.counts, np.uint16)


class LightSummary(NamedTuple):
    """vxrt_light_summary: solid and exposed voxels of the box, its empty voxels by sky and by block level (16 entries
    each), the sums of the two channels' levels, and the emitter entries by class"""
    solid: int
    exposed: int
    hist_sky: tuple
    hist_block: tuple
    sum_sky: int
    sum_block: int
    emitters_used: int
    emitters_solid: int
    emitters_far: int
    emitters_invalid: int


@dataclass
class LightField(_LazyResult):
    """The result of Context.light_field: ``levels`` one byte (sky << 4 | block) per voxel in region order on the device (a
    numpy uint8 [x, y, z] grid from light_field_host), ``summary`` a LightSummary."""
    origin: tuple
    dims: tuple
    channels: int
    levels: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> LightSummary:
        """the summary; for a device field this waits for the call's stream"""
        v = self._words()
        return LightSummary(v[0], v[1], tuple(v[2:18]), tuple(v[18:34]), v[34] | v[35] << 32, v[36] | v[37] << 32, *v[38:42])

    def grid(self) -> np.ndarray:
        """the packed levels as a numpy uint8 [x, y, z] grid (a device field is copied to the host)"""
        return self._xyz(self.levels, np.uint8)

    def sky(self) -> np.ndarray:
        """the sky levels, 0 .. 15, as a numpy uint8 [x, y, z] grid"""
        return self.grid() >> 4

    def block(self) -> np.ndarray:
        """the block levels, 0 .. 15, as a numpy uint8 [x, y, z] grid"""
        return self.grid() & 15


def _count_mask(counts) -> int:
    """the ``born`` / ``survive`` table of a Rule: an int as it is, an iterable of neighbour counts as their bits"""
    if isinstance(counts, (int, np.integer)):
        return int(counts)
    m = 0
    for c in counts:
        if not 0 <= int(c) < 32:
            raise ValueError("a neighbour count is 0 .. 26")
        m |= 1 << int(c)
    return m


def _mask_words(mask: np.ndarray, dims) -> np.ndarray:
    """a rule's mask, a bool [x, y, z] grid of ``dims``, as region words"""
    mask = np.asarray(mask, bool)
    if tuple(mask.shape) != tuple(dims):
        raise ValueError("mask: a bool [x, y, z] grid of the box's dims")
    return pack_region(mask)


@dataclass
class Rule:
    """A neighbour-count rule (include/vxrt.h, vxrt_rule): an empty voxel with c solid voxels among its ``neighbours``
    (RULE_N6, RULE_N18, RULE_N26) becomes solid when c is in ``born``, a solid one stays solid when c is in ``survive``;
    ``iterations`` steps.  ``born`` / ``survive``: an iterable of counts, or an int with bit c set.  ``scope``: RULE_BOX
    (the box alone changes, everything else is frozen) or RULE_WORLD (the box is a window into the rule run on the whole
    world).  ``outside``: what voxels outside the world count as, 0 or 1."""
    neighbours: int = N.RULE_N26
    born: object = 0
    survive: object = 0
    iterations: int = 1
    scope: int = N.RULE_BOX
    outside: int = 0

    def __post_init__(self):
        self.born, self.survive = _count_mask(self.born), _count_mask(self.survive)

    def _c(self) -> "N.RuleDesc":
        i32 = lambda v: max(-1 << 31, min(int(v), (1 << 31) - 1))  # a value outside int32 is the library's to refuse
        return N.RuleDesc(C.sizeof(N.RuleDesc), i32(self.neighbours), _u32(self.born), _u32(self.survive), i32(self.iterations),
                          i32(self.scope), i32(self.outside), 0)

    @staticmethod
    def count(neighbours: int) -> int:
        """the neighbours of a voxel: 6, 18 or 26"""
        return {N.RULE_N6: 6, N.RULE_N18: 18, N.RULE_N26: 26}[int(neighbours)]

    @classmethod
    def smooth(cls, iterations: int = 1, **kw) -> "Rule":
        """the majority of the 27 voxels around and including each: born with 14 or more solid neighbours of 26, kept with 13"""
        return cls(N.RULE_N26, range(14, 27), range(13, 27), iterations, **kw)

    @classmethod
    def grow(cls, neighbours: int = N.RULE_N26, iterations: int = 1, **kw) -> "Rule":
        """thicken by one voxel: born with any solid neighbour, every solid voxel kept"""
        n = cls.count(neighbours)
        return cls(neighbours, range(1, n + 1), range(0, n + 1), iterations, **kw)

    @classmethod
    def erode(cls, neighbours: int = N.RULE_N26, iterations: int = 1, **kw) -> "Rule":
        """shrink by one voxel: nothing born, a solid voxel kept only when all its neighbours are solid"""
        n = cls.count(neighbours)
        return cls(neighbours, 0, (n,), iterations, **kw)

    @classmethod
    def caves(cls, born_min: int, survive_min: int, iterations: int = 4, **kw) -> "Rule":
        """the cave automaton over noise: born with at least ``born_min`` solid neighbours of 26, kept with ``survive_min``"""
        return cls(N.RULE_N26, range(int(born_min), 27), range(int(survive_min), 27), iterations, **kw)


class RuleSummary(NamedTuple):
    """vxrt_rule_summary over the world voxels of the box: solid before and after, voxels born and died between W_0 and W_n,
    voxels the last step changed (0: a fixed point), and the inclusive world box of the voxels that differ from W_0
    (INT32_MAX / INT32_MIN per axis when none does)"""
    solid_before: int
    solid_after: int
    born: int
    died: int
    changed_last: int
    changed_min: tuple
    changed_max: tuple


@dataclass
class RuleResult(_LazyResult):
    """The result of Context.apply_rule: ``bits`` the box after the rule's steps as region words on the device (a numpy
    bool [x, y, z] grid from apply_rule_host), ``summary`` a RuleSummary."""
    bits: object
    origin: tuple
    dims: tuple
    _summary: object
    _stream: object

    @property
    def summary(self) -> RuleSummary:
        """the summary; for a device result this waits for the call's stream"""
        self._summary = self._host(self._summary, np.uint32)
        box = [int(v) for v in np.asarray(self._summary[6:12]).view(np.int32)]
        return RuleSummary(*(int(v) for v in self._summary[:5]), tuple(box[:3]), tuple(box[3:]))

    def grid(self) -> np.ndarray:
        """the voxels as a bool [x, y, z] numpy grid (device words are copied to the host)"""
        return self._bits(self.bits)

    def stamp(self) -> "Stamp":
        """the result as a STAMP_REPLACE stamp at the box's origin, for edit_stamps"""
        return Stamp(self.origin, self.bits, N.STAMP_REPLACE, self.dims)


@dataclass
class Loose:
    """The parameters of a loose-voxel call (include/vxrt.h, vxrt_loose): ``material`` LOOSE_SAND (falls and slides) or
    LOOSE_WATER (also spreads sideways); ``steps`` 1 .. LOOSE_MAX_STEPS; ``edge``: LOOSE_WALL (the box's faces hold the
    material) or LOOSE_OPEN (what leaves the box through an empty voxel is gone); ``phase``: the number of the call's first
    step -- carry it across calls: the phase of the next call is this one's plus its steps."""
    material: int = N.LOOSE_SAND
    steps: int = 1
    edge: int = N.LOOSE_WALL
    phase: int = 0

    def _c(self) -> "N.LooseDesc":
        i32 = lambda v: max(-1 << 31, min(int(v), (1 << 31) - 1))  # a value outside int32 is the library's to refuse
        return N.LooseDesc(C.sizeof(N.LooseDesc), i32(self.material), i32(self.steps), i32(self.edge), int(self.phase) & 0xFFFFFFFF,
                           (C.c_int32 * 3)(0, 0, 0))


class LooseSummary(NamedTuple):
    """vxrt_loose_summary: the input's valid bits over the box, those of them that are loose voxels (in the world and not on a
    solid), the loose voxels after the steps (fewer only under LOOSE_OPEN), the voxels the last step's passes moved (at rest:
    fell_last = slid_last = 0), and the inclusive world box of the voxels where the new layer differs from the input
    (INT32_MAX / INT32_MIN per axis when none does)"""
    loose_in: int
    loose_start: int
    loose_after: int
    fell_last: int
    slid_last: int
    spread_last: int
    changed_min: tuple
    changed_max: tuple


@dataclass
class LooseResult(_LazyResult):
    """The result of Context.loose_step: ``bits`` the new layer as region words on the device (a numpy bool [x, y, z] grid
    from loose_step_host), ``summary`` a LooseSummary."""
    bits: object
    origin: tuple
    dims: tuple
    _summary: object
    _stream: object

    @property
    def summary(self) -> LooseSummary:
        """the summary; for a device result this waits for the call's stream"""
        self._summary = self._host(self._summary, np.uint32)
        box = [int(v) for v in np.asarray(self._summary[6:12]).view(np.int32)]
        return LooseSummary(*(int(v) for v in self._summary[:6]), tuple(box[:3]), tuple(box[3:]))

    def grid(self) -> np.ndarray:
        """the layer as a bool [x, y, z] numpy grid (device words are copied to the host)"""
        return self._bits(self.bits)

    def stamp(self, mode: int = N.STAMP_UNION) -> "Stamp":
        """the layer as a stamp at the box's origin, for edit_stamps: STAMP_UNION makes the loose voxels solid"""
        return Stamp(self.origin, self.bits, mode, self.dims)


@dataclass(frozen=True)
class Orientation:
    """One of the 48 orientations of a stamp (include/vxrt.h, vxrt_orientation): destination axis k runs along source axis
    ``axis[k]``, against it when bit k of ``flip`` is set.  Every method goes through the library's C helpers."""
    axis: tuple = (0, 1, 2)
    flip: int = 0

    def _c(self) -> "N.OrientationDesc":
        d = N.OrientationDesc()
        d.axis = (C.c_int32 * 3)(*[max(-(1 << 31), min(int(a), (1 << 31) - 1)) for a in self.axis])
        d.flip = _u32(self.flip)
        return d

    @staticmethod
    def _of(d: "N.OrientationDesc") -> "Orientation":
        return Orientation(tuple(int(a) for a in d.axis), int(d.flip))

    @staticmethod
    def rotation(axis: int, turns: int = 1) -> "Orientation":
        """``turns`` right-handed quarter turns about ``axis`` (vxrt_orientation_rotation); any integer, taken mod 4"""
        out, t = N.OrientationDesc(), int(turns)
        t = t if -(1 << 31) <= t < 1 << 31 else t % 4  # (the library reduces every int it can be given)
        _helper_ok(N.load().vxrt_orientation_rotation(int(axis), t, C.byref(out)), "rotation axis")
        return Orientation._of(out)

    @staticmethod
    def mirror(axis: int) -> "Orientation":
        """the mirror image along ``axis``"""
        if axis not in (0, 1, 2):
            raise ValueError("mirror axis: 0, 1 or 2")
        return Orientation((0, 1, 2), 1 << axis)

    def then(self, other: "Orientation") -> "Orientation":
        """this orientation first, then ``other`` (vxrt_orientation_compose)"""
        a, b, out = self._c(), other._c(), N.OrientationDesc()
        _helper_ok(N.load().vxrt_orientation_compose(C.byref(a), C.byref(b), C.byref(out)), "orientation")
        return Orientation._of(out)

    def inverse(self) -> "Orientation":
        a, out = self._c(), N.OrientationDesc()
        _helper_ok(N.load().vxrt_orientation_inverse(C.byref(a), C.byref(out)), "orientation")
        return Orientation._of(out)

    def dims(self, src_dims) -> tuple:
        """the destination dims of a stamp of ``src_dims`` (vxrt_orientation_dims)"""
        a, out = self._c(), (C.c_int32 * 3)()
        _helper_ok(N.load().vxrt_orientation_dims(C.byref(a), _i3(src_dims), out), "orientation")
        return tuple(int(v) for v in out)

    def voxel(self, p, src_dims) -> tuple:
        """where source voxel ``p`` of a stamp of ``src_dims`` lands (vxrt_orientation_voxel)"""
        a, out = self._c(), (C.c_int32 * 3)()
        _helper_ok(N.load().vxrt_orientation_voxel(C.byref(a), _i3(src_dims), _i3(p), out), "orientation")
        return tuple(int(v) for v in out)

    @property
    def is_rotation(self) -> bool:
        a = self._c()
        rc = N.load().vxrt_orientation_is_rotation(C.byref(a))
        _helper_ok(min(rc, 0), "orientation")
        return rc == 1

    @staticmethod
    def all():
        """the 48 orientations"""
        import itertools
        for axis in itertools.permutations((0, 1, 2)):
            for flip in range(8):
                yield Orientation(axis, flip)

    @staticmethod
    def rotations():
        """the 24 rotations among them"""
        return (o for o in Orientation.all() if o.is_rotation)


def _helper_ok(rc: int, what: str) -> None:
    """a host-only helper of the library refused its arguments"""
    if rc != 0:
        raise ValueError("invalid " + what)


class TransformSummary(NamedTuple):
    """vxrt_transform_summary: the set voxels, and their inclusive bounds in destination coordinates (INT32_MAX / INT32_MIN
    per axis when there is none)"""
    voxels: int
    set_min: tuple
    set_max: tuple


@dataclass
class TransformedStamp(_LazyResult):
    """The result of Context.transform_stamp: ``bits`` the turned region words on the device (a numpy bool [x, y, z] grid
    from transform_stamp_host), ``dims`` the destination dims, ``summary`` a TransformSummary or None."""
    bits: object
    dims: tuple
    orientation: Orientation
    _summary: object
    _stream: object

    @property
    def summary(self) -> "TransformSummary | None":
        """the summary; for a device result this waits for the call's stream"""
        if self._summary is None:
            return None
        self._summary = self._host(self._summary, np.uint32)
        box = [int(v) for v in np.asarray(self._summary[2:8]).view(np.int32)]
        return TransformSummary(int(self._summary[0]) | int(self._summary[1]) << 32, tuple(box[:3]), tuple(box[3:]))

    def grid(self) -> np.ndarray:
        """the voxels as a bool [x, y, z] numpy grid (device words are copied to the host)"""
        return self._bits(self.bits)

    def stamp(self, origin, mode: int = N.STAMP_REPLACE) -> "Stamp":
        """the result as a stamp at ``origin``, for edit_stamps"""
        return Stamp(_ints(origin), self.bits, mode, self.dims)

    def piece(self) -> "Piece":
        """the result as a piece, for place_pieces"""
        return Piece(self.bits, self.dims)


class DistanceSummary(NamedTuple):
    """vxrt_distance_summary: voxels of the box that are targets, values 1 .. radius^2, DIST_FAR values, the largest value
    that is not DIST_FAR, the sum of the values that are not DIST_FAR"""
    zero: int
    near: int
    far: int
    max_d2: int
    sum_d2: int


@dataclass
class DistanceField(_LazyResult):
    """The result of Context.distance_field: ``dist2`` one two-byte value per voxel in region order on the device (a numpy
    uint16 [x, y, z] grid from distance_field_host), ``summary`` a DistanceSummary."""
    origin: tuple
    dims: tuple
    radius: int
    mode: int
    dist2: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> DistanceSummary:
        """the summary; for a device field this waits for the call's stream"""
        w = self._words()
        return DistanceSummary(*w[:4], w[4] | w[5] << 32)

    def grid(self) -> np.ndarray:
        """the field as a numpy uint16 [x, y, z] grid (a device field is copied to the host)"""
        return self._xyz(self.dist2, np.uint16)


class ReprojectSummary(NamedTuple):
    """vxrt_reproject_summary: hit pixels, and of them those that took over a history, those whose surface point lay outside
    the previous frame, and those the previous frame showed another face at (disocclusions); hit is the sum of the three"""
    hit: int
    reused: int
    offscreen: int
    rejected: int


@dataclass
class Reprojected(_LazyResult):
    """The result of Context.reproject_frame: ``history`` float32 (height, width, 4) records {r, g, b, frames in the mean} --
    the ``history`` argument of the next frame's call --, ``color`` float32 (height, width, 3) its rgb, device tensors;
    ``dims`` is (width, height).  ``summary`` is a ReprojectSummary, or None when the call was made without one."""
    dims: tuple
    history: object
    color: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> ReprojectSummary | None:
        """the summary; the first read waits for the call's stream"""
        return None if self._summary is None else ReprojectSummary(*self._words()[:4])


class LightFrameSummary(NamedTuple):
    """vxrt_light_frame_summary: hit pixels, and of them those whose front cell lies in the light box (with levels given),
    those with a solid cell beside their front cell (some corner with fewer than three open neighbours), and those that no
    light reaches (S == 0 and Bk == 0)"""
    hit: int
    in_box: int
    occluded: int
    dark: int


@dataclass
class LitFrame(_LazyResult):
    """The result of Context.light_frame: ``color`` float32 (height, width, 3), ``terms`` float32 (height, width, 3) holding
    (S, Bk, A) per pixel or None, device tensors; ``dims`` is (width, height).  ``summary`` is a LightFrameSummary, or None
    when the call was made without one."""
    dims: tuple
    color: object
    terms: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> LightFrameSummary | None:
        """the summary; the first read waits for the call's stream"""
        return None if self._summary is None else LightFrameSummary(*self._words()[:4])


@dataclass
class Sky:
    """vxrt_sky_params without the camera: the default is a clear daytime sky.  ``flags``: SKY_CLOUDS or 0.  Colours are
    display-space rgb, >= 0.  ``sun_dir`` points towards the sun (any length); the glow around it is
    ``glow_strength`` * max(cos, 0) ^ (2 ^ ``glow_log2``), the disc is full inside ``cos_inner`` and gone outside
    ``cos_outer``.  Below the horizon the colour runs from ``horizon`` to ``ground`` over 1 / ``ground_fade`` of d.y.
    Clouds: ``octaves`` (1 .. 6) of value noise of seed ``seed`` on the plane y = ``cloud_y``, ``cloud_scale`` noise cells per
    voxel, shifted by ``cloud_offset`` (move it to make them drift), not beyond ``cloud_max_t`` along the ray; ``cloud_cover``
    0 .. 1 is how much of the sky they take, ``cloud_sharp`` how hard their edge is, ``cloud_fade`` how fast they fade in
    above the horizon.  Fog: starts ``fog_start`` voxels from the camera, f = x / (1 + x) with x = distance *
    ``fog_density``, at most ``fog_max`` (0 .. 1)."""
    flags: int = 0
    glow_log2: int = 3
    octaves: int = 4
    seed: int = 1
    zenith: tuple = (0.18, 0.38, 0.80)
    horizon: tuple = (0.70, 0.82, 0.95)
    ground: tuple = (0.30, 0.28, 0.25)
    sun_color: tuple = (1.0, 0.95, 0.80)
    cloud_color: tuple = (1.0, 1.0, 1.0)
    sun_dir: tuple = (0.577, 0.577, 0.577)
    glow_strength: float = 0.35
    ground_fade: float = 4.0
    cos_inner: float = 0.9995
    cos_outer: float = 0.9985
    cloud_y: float = 400.0
    cloud_scale: float = 0.004
    cloud_offset: tuple = (0.0, 0.0)
    cloud_max_t: float = 20000.0
    cloud_cover: float = 0.5
    cloud_sharp: float = 3.0
    cloud_fade: float = 6.0
    fog_start: float = 64.0
    fog_density: float = 0.0015
    fog_max: float = 0.85

    def _c(self, cam, ortho: bool = False) -> "N.SkyParams":
        p = N.SkyParams(struct_size=C.sizeof(N.SkyParams), ortho=1 if ortho else 0, flags=_u32(self.flags), glow_log2=_u32(self.glow_log2),
                        octaves=_u32(self.octaves), seed=int(self.seed) & 0xFFFFFFFF)
        for name in ("zenith", "horizon", "ground", "sun_color", "cloud_color", "sun_dir"):
            setattr(p, name, _f3(getattr(self, name)))
        for name in ("glow_strength", "ground_fade", "cos_inner", "cos_outer", "cloud_y", "cloud_scale", "cloud_max_t", "cloud_cover",
                     "cloud_sharp", "cloud_fade", "fog_start", "fog_density", "fog_max"):
            setattr(p, name, float(getattr(self, name)))
        p.cloud_offset = (C.c_float * 2)(*[float(v) for v in self.cloud_offset])
        _pose(p.cam, cam)
        return p


class SkySummary(NamedTuple):
    """vxrt_sky_summary: miss and hit pixels; of the misses those below the horizon, those the sun disc touches and those
    with a cloud; of the hits those the fog changed"""
    miss: int
    hit: int
    ground: int
    sun: int
    cloud: int
    fogged: int


@dataclass
class SkyFrame(_LazyResult):
    """The result of Context.sky_frame: ``color`` float32 (height, width, 3), a device tensor; ``dims`` is (width, height).
    ``summary`` is a SkySummary, or None when the call was made without one."""
    dims: tuple
    color: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> SkySummary | None:
        """the summary; the first read waits for the call's stream"""
        return None if self._summary is None else SkySummary(*self._words()[:6])


class MaterialRules(NamedTuple):
    """vxrt_material_rules: ``bands`` a sequence of up to eight (y_from, top, under, deep, under_depth) rows in ascending
    y_from, the first None or -2^31 -- the voxels of a band with no solid voxel above them get ``top``, those with 1 ..
    ``under_depth`` (0 .. 15) above them ``under``, the rest ``deep``; material ids are 1 .. 255"""
    bands: tuple

    def _c(self, paint_box=((0, 0, 0), (1, 1, 1))) -> "N.MaterialRulesDesc":
        rows = list(self.bands)
        r = N.MaterialRulesDesc(struct_size=C.sizeof(N.MaterialRulesDesc), n_bands=_u32(len(rows)))
        for i, (y_from, top, under, deep, depth) in enumerate(rows[:N.MATERIAL_MAX_BANDS]):
            b = r.bands[i]
            b.y_from = -(1 << 31) if y_from is None else int(y_from)
            # (a value outside a byte is the library's to refuse: 0 is no material, 255 no depth)
            b.top, b.under, b.deep = (int(v) if 0 <= int(v) <= 255 else 0 for v in (top, under, deep))
            b.under_depth = int(depth) if 0 <= int(depth) <= 255 else 255
        r.paint_origin, r.paint_dims = _i3(paint_box[0]), _i3(paint_box[1])
        return r


class Palette:
    """The 256 entries of vxrt_material and the atlas: ``tints`` float32 (256, 3) (entry m belongs to material m; default
    white), ``tiles`` uint16 (256, 3) holding the atlas tile of the top, side and bottom faces (default MATERIAL_NO_TILE: no
    texture), ``atlas`` an optional uint8 array [n_tiles, T, T, 4] of RGBA8 texels, rows top-down, T a power of two up to 64.
    The first material_frame call with a palette copies it to the device; to capture such a call in a graph, make one eager
    call with the same Palette first."""

    def __init__(self, tints=None, tiles=None, atlas=None):
        self.tints = np.ones((256, 3), np.float32) if tints is None else np.ascontiguousarray(tints, np.float32).reshape(256, 3)
        self.tiles = np.full((256, 3), N.MATERIAL_NO_TILE, np.uint16) if tiles is None else np.ascontiguousarray(tiles, np.uint16).reshape(256, 3)
        self.atlas = None
        self._dev = {}
        self.n_tiles, self.tile_shift = 0, 0
        if atlas is not None:
            a = np.ascontiguousarray(atlas, np.uint8)
            if a.ndim != 4 or a.shape[3] != 4 or a.shape[1] != a.shape[2] or a.shape[1] < 1 or a.shape[1] & (a.shape[1] - 1):
                raise ValueError("atlas: uint8 [n_tiles, T, T, 4] with T a power of two")
            self.atlas, self.n_tiles, self.tile_shift = a, int(a.shape[0]), int(a.shape[1]).bit_length() - 1

    def set(self, material: int, tint=(1.0, 1.0, 1.0), top=N.MATERIAL_NO_TILE, side=None, bottom=None) -> "Palette":
        """entry ``material``: its tint and its tiles (``side`` and ``bottom`` default to ``top``)"""
        self.tints[material] = tint
        self.tiles[material] = (top, top if side is None else side, top if bottom is None else bottom)
        self._dev = {}
        return self

    def _device(self, call: "_Call") -> tuple:
        """(entries, atlas or None) as device tensors on the call's device: uploaded by the first call that uses the palette
        there and kept, so that later calls -- a captured one among them -- copy nothing.  ``set`` drops them; an array
        changed in place needs a new Palette."""
        if call.dev not in self._dev:
            atlas = self.atlas_words()
            self._dev[call.dev] = (call.upload(self.entries()), call.upload(atlas) if atlas is not None else None)
        return tuple(None if t is None else call.reads(t) for t in self._dev[call.dev])

    def entries(self) -> np.ndarray:
        """the 256 entries as the library reads them: 5 words each"""
        e = np.zeros((256, 5), np.uint32)
        e[:, :3] = self.tints.view(np.uint32)
        t = self.tiles.astype(np.uint32)
        e[:, 3] = t[:, 0] | t[:, 1] << 16
        e[:, 4] = t[:, 2]
        return e

    def atlas_words(self):
        """the atlas as packed texels (r in the low byte), or None"""
        return None if self.atlas is None else self.atlas.reshape(-1, 4).view(np.uint32).reshape(-1).copy()


class MaterialSummary(NamedTuple):
    """vxrt_material_summary: solid voxels of the box, those whose material came from paint, those with no solid voxel above
    them, and the voxels by output byte (hist[0]: the empty ones)"""
    solid: int
    painted: int
    top: int
    hist: tuple


@dataclass
class MaterialField(_LazyResult):
    """The result of Context.material_field: ``materials`` one byte per voxel in region order on the device (a numpy uint8
    [x, y, z] grid from material_field_host), ``summary`` a MaterialSummary."""
    origin: tuple
    dims: tuple
    materials: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> MaterialSummary:
        """the summary; for a device field this waits for the call's stream"""
        v = self._words()
        return MaterialSummary(v[0], v[1], v[2], tuple(v[4:260]))

    def grid(self) -> np.ndarray:
        """the bytes as a numpy uint8 [x, y, z] grid (a device field is copied to the host)"""
        return self._xyz(self.materials, np.uint8)


class MaterialFrameSummary(NamedTuple):
    """vxrt_material_frame_summary: hit pixels, and of them those whose material came from paint, those that show a voxel
    with no solid voxel above it, and those that loaded a texel"""
    hit: int
    painted: int
    top: int
    textured: int


@dataclass
class MaterialFrame(_LazyResult):
    """The result of Context.material_frame: ``color`` float32 (height, width, 3), ``materials`` uint8 (height, width) or
    None, device tensors; ``dims`` is (width, height).  ``summary`` is a MaterialFrameSummary, or None when the call was made
    without one."""
    dims: tuple
    color: object
    materials: object
    _summary: object
    _stream: object

    @property
    def summary(self) -> MaterialFrameSummary | None:
        """the summary; the first read waits for the call's stream"""
        return None if self._summary is None else MaterialFrameSummary(*self._words()[:4])


class NavAgent(NamedTuple):
    """vxrt_nav_agent: a width x height x width box of cells standing on its minimum corner, that steps up at most
    ``climb`` cells and down at most ``drop``"""
    width: int = 1
    height: int = 2
    climb: int = 1
    drop: int = 3

    def _c(self):
        return (C.c_int32 * 4)(int(self.width), int(self.height), int(self.climb), int(self.drop))


class NavSummary(NamedTuple):
    """vxrt_nav_summary"""
    nodes: int
    goals_used: int
    goals_ignored: int
    reached: int
    max_dist_found: int
    levels: int
    tiles_total: int
    tile_visits: int


class NavPaths(NamedTuple):
    """The result of NavField.paths: ``cells`` (n, max_steps + 1, 3) int32 or None, ``lengths`` and ``status`` (NAV_AT_GOAL,
    NAV_NO_PATH, NAV_TRUNCATED, NAV_OUTSIDE) per start, as device tensors"""
    cells: object
    lengths: object
    status: object


def nav_move(code: int, agent: NavAgent) -> tuple:
    """(dx, dy, dz) of a next code of a field for ``agent`` (include/vxrt.h: 1 + direction * (1 + climb + drop) + dy index,
    directions +x, -x, +z, -z, dy in the order 0, 1 .. climb, -1 .. -drop)"""
    per = 1 + agent.climb + agent.drop
    if not 1 <= code <= 4 * per:
        raise ValueError("not a move code: %d" % code)
    k, i = divmod(code - 1, per)
    dy = 0 if i == 0 else (i if i <= agent.climb else -(i - agent.climb))
    return ((1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1))[k][0], dy, ((1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1))[k][2]


@dataclass
class NavField:
    """The result of Context.nav_field: ``walkable`` the node bits (region words on the device; a bool grid from
    nav_field_host), ``next`` one code per cell in region order (uint8), ``dist`` one uint32 per cell (0xFFFFFFFF
    unreachable) or None, ``summary`` a NavSummary."""
    origin: tuple
    dims: tuple
    agent: NavAgent
    walkable: object
    next: object
    dist: object
    summary: NavSummary
    ctx: object = field(default=None, repr=False)

    def paths(self, starts, max_steps: int, cells: bool = True, stream: int | None = None) -> NavPaths:
        """Follow the next codes from each world cell of ``starts`` ((n, 3)) for at most ``max_steps`` moves
        (vxrt_nav_paths; asynchronous on ``stream``, default torch's current stream).  Needs the device field of
        Context.nav_field."""
        if not hasattr(self.next, "data_ptr"):
            raise ValueError("paths needs the device field of Context.nav_field")
        call = _Call(self.ctx, stream)
        i32 = call.torch.int32
        st = np.ascontiguousarray(np.asarray(starts, np.int32).reshape(-1, 3))
        n = st.shape[0]
        st = call.upload(st) if n else call.out(3, 4, i32)  # never NULL: n == 0 is the call's no-op
        out = call.torch.empty((max(n, 1), int(max_steps) + 1, 3), dtype=i32, device=call.dev) if cells else None
        lengths, status = call.out(n, 4, i32), call.out(n, 4, i32)

        class _Desc(C.Structure):
            _fields_ = [("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("agent", C.c_int32 * 4), ("d_next", C.c_void_p)]
        desc = _Desc(_i3(self.origin), _i3(self.dims), self.agent._c(), call.reads(self.next).data_ptr())
        call.launch(self.ctx._L.vxrt_nav_paths, C.byref(desc), _ptr(st), n, int(max_steps), _ptr(out), _ptr(lengths), _ptr(status))
        return NavPaths(out[:n] if cells else None, lengths[:n], status[:n])


def _bodies_np(bodies) -> np.ndarray:
    if isinstance(bodies, (list, tuple)) and (len(bodies) == 0 or isinstance(bodies[0], Body)):
        bodies = Body.pack(bodies)
    b = np.ascontiguousarray(bodies, np.float32)
    if b.ndim != 2 or b.shape[1] != 9:
        raise ValueError("bodies must be (n, 9) float32: lo[3], hi[3], delta[3]")
    return b


def _bodies_dev(bodies):
    import torch
    if bodies.dtype != torch.float32 or bodies.dim() != 2 or bodies.shape[1] != 9:
        raise ValueError("bodies must be an (n, 9) float32 tensor: lo[3], hi[3], delta[3]")
    return bodies.contiguous()


class _Call:
    """One device query: its stream, its buffers and its one exit.  The four things every query decides the same way:
    which tensors must outlive the Python call (``work``, ``upload``, ``reads`` note them and ``launch`` records them on the
    call's stream, so that torch's allocator does not hand their memory out again before the stream has passed the call),
    how a host array reaches the device ordered before that stream (``upload`` and ``launch``), which tensors of the
    caller's are accepted (``fits``), and what a placeholder for a refused or empty call looks like (``out``, ``work``)."""

    def __init__(self, ctx: "Context", stream):
        import torch
        self.torch, self.ctx = torch, ctx
        self.dev = "cuda:%d" % ctx.device
        self.s = _stream(stream)  # the raw handle the library takes
        self._stream = None
        self._held = []
        self._uploaded = False

    @property
    def stream(self):
        """the call's stream as torch's"""
        if self._stream is None:
            self._stream = self.torch.cuda.ExternalStream(self.s, device=self.dev)
        return self._stream

    def fits(self, t, count: int, elem_size: int, what: str, any_size: bool = False):
        """``t``, the caller's: a contiguous device tensor of at least ``count`` elements of ``elem_size`` bytes, or with
        ``any_size`` of as many bytes in elements of any size; ValueError(``what``) otherwise"""
        if any_size:
            enough = t.numel() * t.element_size() >= count * elem_size
        else:
            enough = t.element_size() == elem_size and t.numel() >= count
        if not (enough and t.is_cuda and t.is_contiguous()):  # data_ptr() of a strided tensor is not a dense buffer
            raise ValueError(what)
        return t

    def out(self, count: int, elem_size: int, dtype, given=None, what: str = "", any_size: bool = False):
        """an output of ``count`` elements: a new tensor (one element for a count of 0, never NULL), or ``given`` if it fits"""
        if given is None:
            return self.torch.empty(max(count, 1), dtype=dtype, device=self.dev)
        return self.fits(given, count, elem_size, what, any_size)

    def work(self, nbytes: int, given=None, what: str = "", least: int = 4):
        """the workspace: new bytes (``least`` for a size of 0, never NULL), or ``given`` if it holds ``nbytes``"""
        if given is None:
            return self.reads(self.torch.empty(max(nbytes, least), dtype=self.torch.uint8, device=self.dev))
        return self.reads(self.fits(given, nbytes, 1, what, any_size=True))

    def summary(self, nwords: int):
        return self.torch.zeros(nwords, dtype=self.torch.int32, device=self.dev)

    # ---- what the frame stages share (denoise_frame, reproject_frame, light_frame, sky_frame, material_frame)
    def fits_f32(self, t, count: int, what: str):
        """``t``, the caller's, if it fits ``count`` float32 elements; ValueError(``what``) otherwise"""
        if self.fits(t, count, 4, what).dtype != self.torch.float32:
            raise ValueError(what)
        return t

    def frame_inputs(self, color, keys, *hit_aov):
        """the colour tensor, the keys and (a stage that decodes hit indices) the hit AOV of a frame, checked and noted as
        read; returns (width, height, width * height)"""
        if color.dim() != 3 or color.shape[2] != 3 or color.dtype != self.torch.float32 or not color.is_contiguous():
            raise ValueError("color: a contiguous float32 device tensor (height, width, 3)")
        height, width = int(color.shape[0]), int(color.shape[1])
        n = width * height
        self.reads(color)
        self.reads(self.fits(keys, n, 4, "keys: a contiguous device tensor of width * height four-byte elements"))
        for hit in hit_aov:
            self.reads(self.fits(hit, n, 8, "hit_aov: a contiguous device tensor of width * height eight-byte elements"))
        return width, height, n

    def frame_outputs(self, color, n: int, out, fb):
        """the colour output of a frame of ``n`` pixels -- a new tensor like ``color``, or ``out`` if it fits -- with ``fb``,
        where one is given, checked"""
        if out is None:
            out = self.torch.empty_like(color)
        else:
            self.fits_f32(out, 3 * n, "out: a contiguous float32 device tensor (height, width, 3)")
        if fb is not None:
            self.fits(fb, n, 4, "fb: a contiguous device tensor of width * height * 4 bytes", any_size=True)
        return out

    def frame_plane(self, given, shape, dtype, what: str):
        """an optional output plane of a frame: None for False, a new tensor of ``shape`` for True, else ``given``, the
        caller's, if it holds ``shape`` elements of ``dtype``'s size (a float32 plane: of that type)"""
        if given is True or given is False:
            return self.torch.empty(shape, dtype=dtype, device=self.dev) if given else None
        count = int(np.prod(shape))
        return self.fits_f32(given, count, what) if dtype == self.torch.float32 else self.fits(given, count, 1, what)

    def reads(self, t):
        """``t``, a device tensor the launch reads or scratches: the caller's, or a temporary dropped when the method returns"""
        self._held.append(t)
        return t

    def upload(self, a: np.ndarray):
        """a host array of four-byte values as an int32 device tensor of its shape, copied on torch's current stream"""
        self._uploaded = self._uploaded or a.size > 0
        return self.reads(self.torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(self.dev))

    def upload_bytes(self, a: np.ndarray):
        """a host array of bytes as a uint8 device tensor of its shape, copied on torch's current stream"""
        self._uploaded = self._uploaded or a.size > 0
        return self.reads(self.torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).to(self.dev))

    def launch(self, fn, *args) -> None:
        """``fn(ctx, *args, stream)`` checked.  An upload was queued on torch's current stream, which need not be the call's:
        the host waits for it first.  Afterwards every tensor noted is recorded on the call's stream."""
        if self._uploaded:
            self.torch.cuda.current_stream(self.dev).synchronize()
            self._uploaded = False
        N.check(fn(self.ctx._h, *args, self.s))
        for t in self._held:
            t.record_stream(self.stream)


def _ints(v) -> tuple:
    return tuple(int(x) for x in v)


def _box(origin, dims):
    """a box as the results carry it: (origin, dims) as tuples of ints"""
    return _ints(origin), _ints(dims)


def _counts(dims, accepted) -> tuple:
    """(voxels, region words) of a box the call's contract accepts -- ``accepted``: its workspace size or word count, 0 for
    a box it refuses -- else (0, 0): the buffers are then one-element placeholders and the library does the refusing"""
    return (dims[0] * dims[1] * dims[2], region_words(dims)) if accepted else (0, 0)


def _grid(a: np.ndarray, dims) -> np.ndarray:
    """one value per voxel in region order (x fastest, then y, then z) -> [x, y, z]"""
    return a[: dims[0] * dims[1] * dims[2]].reshape(dims[::-1]).transpose(2, 1, 0)


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def _u32(v) -> int:
    """an argument of a uint32 parameter: a value outside it is the library's to refuse, not ctypes' to wrap"""
    v = int(v)
    return v if 0 <= v < 1 << 32 else 0xFFFFFFFF


def region_words(dims) -> int:
    """Words of a region of ``dims`` voxels (vxrt_region_words): ceil(dims[0] / 32) * dims[1] * dims[2]; 0 for bad dims."""
    return int(N.load().vxrt_region_words(_i3(dims)))


def pack_region(vox) -> np.ndarray:
    """bool [x, y, z] -> region words (uint32): each x row padded to a multiple of 32 bits, rows y fastest, then z."""
    v = np.asarray(vox, bool)
    X, Y, Z = v.shape
    wpr = (X + 31) // 32
    rows = np.zeros((Z, Y, wpr * 32), bool)
    rows[:, :, :X] = v.transpose(2, 1, 0)
    return np.packbits(rows, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


def unpack_region(words, dims) -> np.ndarray:
    """region words (uint32 numpy array, or a tensor of int32 / uint32) -> bool [x, y, z]"""
    if hasattr(words, "cpu"):
        words = words.cpu().numpy()
    X, Y, Z = (int(d) for d in dims)
    wpr = (X + 31) // 32
    w = np.ascontiguousarray(words).view(np.uint32)[: wpr * Y * Z].reshape(Z, Y, wpr)
    bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[:, :, :X]
    return bits.astype(bool).transpose(2, 1, 0)


def grid_is_wide(cdims) -> bool:
    """The rule of csrc/vxrt_device.hpp (grid_is_wide): a coarse grid beyond the tracer's packed step counters -- more than
    1020 / 508 / 1020 cells, or one a single walk could cross in MAX_STEPS iterations -- runs the WIDE instantiation."""
    cx, cy, cz = (int(c) for c in cdims)
    return cx > 1020 or cz > 1020 or cy > 508 or cx + cy + cz + 4 >= 2048


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_cuda:
            raise ValueError("device tensor expected")
        return x.data_ptr()
    raise TypeError(f"cannot take a device pointer from {type(x)}")


def _stream(s):
    if s is not None:
        return s
    import torch
    return torch.cuda.current_stream().cuda_stream
