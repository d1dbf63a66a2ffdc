"""ctypes view of the C ABI in include/vxrt.h.  The library is required: nothing here falls back to a
CPU path -- a missing or unloadable libvxrt.so raises."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

EMPTY_SLOT = 0xFFFFFFFF
MAX_STEPS = 2048
GEN_HASH_HEIGHTFIELD, GEN_PERLIN_REF, GEN_INT_TERRAIN = 0, 1, 2
MODE_SHADED, MODE_DEBUG = 0, 1

# every symbol include/vxrt.h declares
EXPORTS = [
    "vxrt_abi_version", "vxrt_create", "vxrt_destroy", "vxrt_last_error", "vxrt_synchronize", "vxrt_set_kernel_variant", "vxrt_kernel_for_launch",
    "vxrt_render_specialisation",
    "vxrt_has_experiments", "vxrt_set_persistent_waves_per_cu", "vxrt_debug_guard_pretend_no_slack",
    "vxrt_upload_world", "vxrt_build_world_procedural", "vxrt_world_info_get", "vxrt_download_world",
    "vxrt_save_world", "vxrt_load_world", "vxrt_world_file_info",
    "vxrt_set_environment", "vxrt_set_fov", "vxrt_set_ortho_window_size", "vxrt_get_directions",
    "vxrt_render_flags_default", "vxrt_render", "vxrt_render_views", "vxrt_compact_rows", "vxrt_frame_stats_get",
    "vxrt_loop_counters_get",
    "vxrt_deinterleave_strips", "vxrt_deinterleave_views", "vxrt_trace_batch", "vxrt_trace_batch_host",
    "vxrt_set_batch_max_steps", "vxrt_stream_open", "vxrt_stream_focus", "vxrt_stream_resident", "vxrt_stream_close",
    "vxrt_edit_voxels", "vxrt_edit_reserve",
    "vxrt_region_words", "vxrt_read_region", "vxrt_read_region_host", "vxrt_edit_stamps",
    "vxrt_move_boxes", "vxrt_overlap_boxes", "vxrt_move_boxes_host", "vxrt_overlap_boxes_host",
    "vxrt_islands_workspace_bytes", "vxrt_find_islands", "vxrt_find_islands_host",
    "vxrt_place_pieces", "vxrt_place_pieces_host",
    "vxrt_orientation_rotation", "vxrt_orientation_compose", "vxrt_orientation_inverse", "vxrt_orientation_dims",
    "vxrt_orientation_voxel", "vxrt_orientation_is_rotation", "vxrt_transform_stamp", "vxrt_transform_stamp_host",
    "vxrt_nav_workspace_bytes", "vxrt_nav_field", "vxrt_nav_paths", "vxrt_nav_field_host",
    "vxrt_distance_workspace_bytes", "vxrt_distance_field", "vxrt_distance_field_host",
    "vxrt_voxelize_workspace_bytes", "vxrt_voxelize_mesh", "vxrt_voxelize_mesh_host",
    "vxrt_surface_workspace_bytes", "vxrt_extract_surface", "vxrt_extract_surface_host",
    "vxrt_lod_workspace_bytes", "vxrt_downsample_region", "vxrt_downsample_region_host",
    "vxrt_light_workspace_bytes", "vxrt_light_field", "vxrt_light_field_host",
    "vxrt_rule_workspace_bytes", "vxrt_apply_rule", "vxrt_apply_rule_host",
    "vxrt_loose_workspace_bytes", "vxrt_loose_step", "vxrt_loose_step_host",
    "vxrt_frame_guides", "vxrt_denoise_workspace_bytes", "vxrt_denoise_frame", "vxrt_reproject_frame", "vxrt_light_frame",
    "vxrt_material_field", "vxrt_material_field_host", "vxrt_material_frame", "vxrt_sky_frame",
]
EDIT_BOX, EDIT_SPHERE = 0, 1
EDIT_MAX_OPS = 1024
STAMP_REPLACE, STAMP_UNION, STAMP_SUBTRACT = 0, 1, 2
BODY_MAX_EXTENT, BODY_MAX_DELTA = 64, 64
BODY_BLOCKED_X, BODY_BLOCKED_Y, BODY_BLOCKED_Z, BODY_INVALID = 1, 2, 4, 8
ISLAND_ANCHOR_X_LO, ISLAND_ANCHOR_X_HI, ISLAND_ANCHOR_Y_LO, ISLAND_ANCHOR_Y_HI = 0x01, 0x02, 0x04, 0x08
ISLAND_ANCHOR_Z_LO, ISLAND_ANCHOR_Z_HI, ISLAND_ANCHOR_FACES, ISLAND_ANCHOR_FLOOR = 0x10, 0x20, 0x3F, 0x40
PLACE_MAX_PIECES, PLACE_MAX_DIM, PLACE_MAX_VOXELS, PLACE_MAX_DIST = 64, 1024, 1 << 24, 4096
PLACED_BLOCKED, PLACED_INVALID = 1, 2
NAV_MAX_GOALS, NAV_NONE, NAV_MAX_STEPS = 4096, 0xFF, 65535
NAV_AT_GOAL, NAV_NO_PATH, NAV_TRUNCATED, NAV_OUTSIDE = 0, 1, 2, 3
DIST_TO_SOLID, DIST_TO_EMPTY, DIST_FAR, DIST_MAX_RADIUS = 0, 1, 0xFFFF, 255
VOX_SURFACE, VOX_SOLID, VOX_FRAC_BITS, VOX_MAX_DIM, VOX_MAX_COORD, VOX_MAX_TRIANGLES = 1, 2, 8, 1024, 1 << 18, 1 << 24
SURF_CAP, SURF_OPEN, SURF_MAX_DIM = 0, 1, 1024
LOD_MAX_SHIFT = 5
LIGHT_SKY, LIGHT_BLOCK, LIGHT_MAX, LIGHT_MAX_EMITTERS = 1, 2, 15, 65536
LF_SMOOTH, LF_OCCLUSION = 1, 2
SKY_CLOUDS, SKY_MAX_GLOW_LOG2, SKY_MAX_OCTAVES = 1, 8, 6
RULE_N6, RULE_N18, RULE_N26, RULE_BOX, RULE_WORLD, RULE_MAX_ITERATIONS = 0, 1, 2, 0, 1, 16
LOOSE_SAND, LOOSE_WATER, LOOSE_WALL, LOOSE_OPEN, LOOSE_MAX_STEPS = 0, 1, 0, 1, 64
TRANSFORM_MAX_WORDS = 1 << 31


class WorldDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("factor", C.c_int32), ("cdims", C.c_int32 * 3), ("nslots", C.c_uint64),
        ("coarse_bits", C.c_void_p), ("brick_slot", C.c_void_p), ("bounds", C.c_void_p), ("pool", C.c_void_p),
    ]


class WorldInfo(C.Structure):
    _fields_ = [("factor", C.c_int32), ("cdims", C.c_int32 * 3), ("ncells", C.c_uint64), ("nslots", C.c_uint64),
                ("hbm_bytes", C.c_uint64)]


class FrameStats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("bounce_rays", C.c_uint64),
                ("primary_hits", C.c_uint64), ("coarse_probes", C.c_uint64), ("brick_entries", C.c_uint64),
                ("fine_probes", C.c_uint64), ("dbg", C.c_uint64 * 13), ("guard_slack_loads", C.c_uint64),
                ("guard_stray_loads", C.c_uint64)]

    def total_rays(self) -> int:
        return int(self.primary_rays + self.shadow_rays + self.bounce_rays)

    def algorithmic_bytes(self, batch: bool = False) -> int:
        """B = Nc*(4+24) + Nb*24 + Nf*4 + P, on the reference's data layout at its load
        granularity (4-B bit word + 24-B Bounds3Df per coarse probe, 24-B VoxelBuffer3D descriptor per brick
        entry, 4-B word per brick probe); P = 4-B pixel store per primary ray (batch: 24 B in + 28 B out)."""
        per_primary = 52 if batch else 4
        return int(self.coarse_probes * 28 + self.brick_entries * 24 + self.fine_probes * 4
                   + self.primary_rays * per_primary)


class StreamStats(C.Structure):
    _fields_ = [("chunks_total", C.c_uint64), ("chunks_occupied", C.c_uint64), ("chunks_resident", C.c_uint64),
                ("bricks_resident", C.c_uint64), ("chunks_loaded", C.c_uint64), ("chunks_evicted", C.c_uint64),
                ("chunks_missing", C.c_uint64), ("bytes_read", C.c_uint64)]


class EditOp(C.Structure):
    """vxrt_edit_op: BOX a = inclusive min voxel, b = inclusive max voxel; SPHERE a = centre, b = (radius, 0, 0)."""
    _fields_ = [("kind", C.c_int32), ("value", C.c_int32), ("a", C.c_int32 * 3), ("b", C.c_int32 * 3)]

    def __repr__(self):
        return "EditOp(kind=%d, value=%d, a=%s, b=%s)" % (self.kind, self.value, list(self.a), list(self.b))


class EditStats(C.Structure):
    _fields_ = [("bricks_touched", C.c_uint64), ("bricks_created", C.c_uint64), ("bricks_freed", C.c_uint64),
                ("bricks_live", C.c_uint64), ("pool_slots", C.c_uint64), ("pool_capacity", C.c_uint64)]


class StampDesc(C.Structure):
    """vxrt_stamp: a dense bit volume (region layout, include/vxrt.h) written at `origin` in `mode`."""
    _fields_ = [("d_bits", C.c_void_p), ("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("mode", C.c_int32),
                ("reserved", C.c_int32)]


class PieceDesc(C.Structure):
    """vxrt_piece: a rigid dense bit volume (region layout, include/vxrt.h) for vxrt_place_pieces."""
    _fields_ = [("d_bits", C.c_void_p), ("dims", C.c_int32 * 3), ("reserved", C.c_int32)]


class OrientationDesc(C.Structure):
    """vxrt_orientation: destination axis k runs along source axis axis[k], against it when bit k of flip is set."""
    _fields_ = [("axis", C.c_int32 * 3), ("flip", C.c_uint32)]


class TransformSummaryDesc(C.Structure):
    """vxrt_transform_summary"""
    _fields_ = [("voxels", C.c_uint64), ("set_min", C.c_int32 * 3), ("set_max", C.c_int32 * 3)]


class RenderFlags(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("mode", C.c_int32), ("checkerboard", C.c_int32), ("shadow", C.c_int32),
        ("bounce_samples", C.c_int32), ("bounce_all_hits", C.c_int32), ("bounce_depth", C.c_int32), ("ortho", C.c_int32),
        ("frame_number", C.c_int64),
        ("strip_rows", C.c_int32), ("strip_count", C.c_int32), ("strip_index", C.c_int32), ("compact", C.c_int32),
        ("collect_stats", C.c_int32), ("tile_schedule", C.c_int32),
        ("d_color_aov", C.c_void_p), ("d_hit_aov", C.c_void_p), ("d_tile_order", C.c_void_p), ("stream", C.c_void_p),
        ("d_accum", C.c_void_p), ("accum_reset", C.c_int32), ("reserved_", C.c_int32),
    ]


class DenoiseParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("color_scale", C.c_float), ("reserved_", C.c_int32)]


class RuleDesc(C.Structure):
    """vxrt_rule: a neighbour-count rule (include/vxrt.h, vxrt_apply_rule)."""
    _fields_ = [("struct_size", C.c_uint32), ("neighbours", C.c_int32), ("born", C.c_uint32), ("survive", C.c_uint32),
                ("iterations", C.c_int32), ("scope", C.c_int32), ("outside", C.c_int32), ("reserved_", C.c_int32)]


class LooseDesc(C.Structure):
    """vxrt_loose: the parameters of a loose-voxel call (include/vxrt.h, vxrt_loose_step)."""
    _fields_ = [("struct_size", C.c_uint32), ("material", C.c_int32), ("steps", C.c_int32), ("edge", C.c_int32),
                ("phase", C.c_uint32), ("reserved_", C.c_int32 * 3)]


class CameraPose(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("fwd", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3)]


class ReprojectParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ortho", C.c_int32), ("max_history", C.c_int32), ("reserved_", C.c_int32),
                ("cur", CameraPose), ("prev", CameraPose)]


class LightFrameParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ortho", C.c_int32), ("flags", C.c_uint32), ("outside_level", C.c_uint32),
                ("sky_floor", C.c_float), ("block_color", C.c_float * 3), ("ao_curve", C.c_float * 4), ("cam", CameraPose),
                ("box_origin", C.c_int32 * 3), ("box_dims", C.c_int32 * 3), ("reserved_", C.c_int32)]


MATERIAL_MAX_BANDS, MATERIAL_NO_TILE, MATERIAL_MAX_TILES, MATERIAL_MAX_TILE_SHIFT = 8, 0xFFFF, 4096, 6


class MaterialBand(C.Structure):
    _fields_ = [("y_from", C.c_int32), ("top", C.c_uint8), ("under", C.c_uint8), ("deep", C.c_uint8), ("under_depth", C.c_uint8)]


class MaterialRulesDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_bands", C.c_uint32), ("bands", MaterialBand * 8), ("paint_origin", C.c_int32 * 3),
                ("paint_dims", C.c_int32 * 3), ("reserved_", C.c_int32)]


class MaterialFrameParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ortho", C.c_int32), ("n_tiles", C.c_uint32), ("tile_shift", C.c_uint32),
                ("cam", CameraPose), ("reserved_", C.c_int32)]


class SkyParams(C.Structure):
    """vxrt_sky_params: the parameters of a sky call (include/vxrt.h, vxrt_sky_frame)."""
    _fields_ = [("struct_size", C.c_uint32), ("ortho", C.c_int32), ("flags", C.c_uint32), ("glow_log2", C.c_uint32), ("octaves", C.c_uint32),
                ("seed", C.c_uint32), ("zenith", C.c_float * 3), ("horizon", C.c_float * 3), ("ground", C.c_float * 3),
                ("sun_color", C.c_float * 3), ("cloud_color", C.c_float * 3), ("sun_dir", C.c_float * 3), ("glow_strength", C.c_float),
                ("ground_fade", C.c_float), ("cos_inner", C.c_float), ("cos_outer", C.c_float), ("cloud_y", C.c_float),
                ("cloud_scale", C.c_float), ("cloud_offset", C.c_float * 2), ("cloud_max_t", C.c_float), ("cloud_cover", C.c_float),
                ("cloud_sharp", C.c_float), ("cloud_fade", C.c_float), ("fog_start", C.c_float), ("fog_density", C.c_float),
                ("fog_max", C.c_float), ("cam", CameraPose), ("reserved_", C.c_int32)]


class View(C.Structure):
    _fields_ = [
        ("d_fb", C.c_void_p), ("origin", C.c_float * 3), ("fwd", C.c_float * 3), ("up", C.c_float * 3),
        ("right", C.c_float * 3), ("frame_number", C.c_int64), ("d_color_aov", C.c_void_p), ("d_hit_aov", C.c_void_p),
    ]


_LIB = None


def lib_path() -> str:
    return _build.LIB_PATH


def load() -> C.CDLL:
    """Load libvxrt.so (building it first if sources are newer).  Raises if that is impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PyTorch ships its own libamdhip64; it must be the HIP runtime of the process before libvxrt.so binds to
    # one, or the two runtimes fight over the device (seen as "no ROCm-capable device is detected").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("VXRT_LIB", _build.LIB_PATH)  # VXRT_LIB: A/B builds of the same library (tools/)
    if path == _build.LIB_PATH:
        # Content-hash staleness check against every source of the library; make/hipcc run only when it is stale, under a
        # lock, into a temporary file renamed into place (build.build_lib).  Normally this process has not touched the GPU
        # yet, so the make child is harmless; under a profiler (whose preload initialises the GPU before Python starts)
        # build beforehand and set VXRT_SKIP_STALE_CHECK=1 so that no child is started here.
        _build.build_lib(force=bool(os.environ.get("VXRT_REBUILD")))
    if not os.path.exists(path):
        raise RuntimeError(f"libvxrt.so not found at {path}; run __graft_entry__.build()")
    L = C.CDLL(path)
    f3 = C.POINTER(C.c_float)
    L.vxrt_abi_version.restype = C.c_int
    L.vxrt_last_error.restype = C.c_char_p
    L.vxrt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.vxrt_destroy.argtypes = [C.c_void_p]
    L.vxrt_synchronize.argtypes = [C.c_void_p]
    L.vxrt_set_kernel_variant.argtypes = [C.c_void_p, C.c_int]
    L.vxrt_has_experiments.restype = C.c_int
    L.vxrt_debug_guard_pretend_no_slack.argtypes = [C.c_void_p, C.c_int]
    L.vxrt_set_persistent_waves_per_cu.argtypes = [C.c_void_p, C.c_int]
    L.vxrt_kernel_for_launch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    L.vxrt_kernel_for_launch.restype = C.c_int
    L.vxrt_render_specialisation.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    L.vxrt_render_specialisation.restype = C.c_int
    L.vxrt_upload_world.argtypes = [C.c_void_p, C.POINTER(WorldDesc)]
    L.vxrt_build_world_procedural.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.vxrt_world_info_get.argtypes = [C.c_void_p, C.POINTER(WorldInfo)]
    L.vxrt_download_world.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_save_world.argtypes = [C.c_void_p, C.c_char_p]
    L.vxrt_load_world.argtypes = [C.c_void_p, C.c_char_p]
    L.vxrt_world_file_info.argtypes = [C.c_char_p, C.POINTER(WorldInfo)]
    L.vxrt_set_environment.argtypes = [C.c_void_p, f3, f3, f3]
    L.vxrt_set_fov.argtypes = [C.c_void_p, C.c_float]
    L.vxrt_set_ortho_window_size.argtypes = [C.c_void_p, C.c_float, C.c_float]
    L.vxrt_get_directions.argtypes = [f3, f3, f3, f3]
    L.vxrt_get_directions.restype = None
    L.vxrt_render_flags_default.argtypes = [C.POINTER(RenderFlags)]
    L.vxrt_render_flags_default.restype = None
    L.vxrt_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, f3, f3, f3, f3, C.POINTER(RenderFlags)]
    L.vxrt_render_views.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(View), C.POINTER(RenderFlags)]
    L.vxrt_compact_rows.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32]
    L.vxrt_compact_rows.restype = C.c_uint32
    L.vxrt_frame_stats_get.argtypes = [C.c_void_p, C.POINTER(FrameStats)]
    L.vxrt_loop_counters_get.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]
    L.vxrt_deinterleave_strips.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_uint64, C.c_void_p, C.c_void_p]
    L.vxrt_deinterleave_views.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64,
                                          C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.vxrt_trace_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.POINTER(FrameStats), C.c_void_p]
    L.vxrt_set_batch_max_steps.argtypes = [C.c_void_p, C.c_int32]
    L.vxrt_stream_open.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.vxrt_stream_focus.argtypes = [C.c_void_p, f3, C.c_float, C.POINTER(StreamStats)]
    L.vxrt_stream_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.vxrt_stream_close.argtypes = [C.c_void_p]
    L.vxrt_edit_voxels.argtypes = [C.c_void_p, C.POINTER(EditOp), C.c_uint32, C.POINTER(EditStats)]
    L.vxrt_edit_reserve.argtypes = [C.c_void_p, C.c_uint64]
    L.vxrt_region_words.restype = C.c_uint64
    L.vxrt_region_words.argtypes = [C.POINTER(C.c_int32)]
    L.vxrt_read_region.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    L.vxrt_read_region_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    L.vxrt_edit_stamps.argtypes = [C.c_void_p, C.POINTER(StampDesc), C.c_uint32, C.POINTER(EditStats)]
    L.vxrt_move_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                  C.c_void_p]
    L.vxrt_overlap_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_move_boxes_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    L.vxrt_overlap_boxes_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.vxrt_islands_workspace_bytes.restype = C.c_uint64
    L.vxrt_islands_workspace_bytes.argtypes = [C.POINTER(C.c_int32)]
    L.vxrt_find_islands.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.vxrt_find_islands_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.vxrt_place_pieces.argtypes = [C.c_void_p, C.POINTER(PieceDesc), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.vxrt_place_pieces_host.argtypes = [C.c_void_p, C.POINTER(PieceDesc), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    po, i3 = C.POINTER(OrientationDesc), C.POINTER(C.c_int32)
    L.vxrt_orientation_rotation.argtypes = [C.c_int, C.c_int, po]
    L.vxrt_orientation_compose.argtypes = [po, po, po]
    L.vxrt_orientation_inverse.argtypes = [po, po]
    L.vxrt_orientation_dims.argtypes = [po, i3, i3]
    L.vxrt_orientation_voxel.argtypes = [po, i3, i3, i3]
    L.vxrt_orientation_is_rotation.argtypes = [po]
    L.vxrt_transform_stamp.argtypes = [C.c_void_p, C.c_void_p, i3, po, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_transform_stamp_host.argtypes = [C.c_void_p, C.c_void_p, i3, po, C.c_void_p, C.c_void_p]
    L.vxrt_nav_workspace_bytes.restype = C.c_uint64
    L.vxrt_nav_workspace_bytes.argtypes = [C.POINTER(C.c_int32), C.c_void_p]
    L.vxrt_nav_field.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_uint32,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_nav_field_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_nav_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    L.vxrt_distance_workspace_bytes.restype = C.c_uint64
    L.vxrt_distance_workspace_bytes.argtypes = [C.POINTER(C.c_int32), C.c_uint32]
    L.vxrt_distance_field.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_distance_field_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_int32,
                                           C.c_void_p, C.c_void_p]
    L.vxrt_voxelize_workspace_bytes.restype = C.c_uint64
    L.vxrt_voxelize_workspace_bytes.argtypes = [C.POINTER(C.c_int32), C.c_uint32]
    L.vxrt_voxelize_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_voxelize_mesh_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32),
                                          C.c_int32, C.c_void_p, C.c_void_p]
    L.vxrt_surface_workspace_bytes.restype = C.c_uint64
    L.vxrt_surface_workspace_bytes.argtypes = [C.POINTER(C.c_int32)]
    L.vxrt_extract_surface.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_extract_surface_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_lod_workspace_bytes.restype = C.c_uint64
    L.vxrt_lod_workspace_bytes.argtypes = [C.POINTER(C.c_int32), C.c_uint32]
    L.vxrt_downsample_region.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_downsample_region_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_light_workspace_bytes.restype = C.c_uint64
    L.vxrt_light_workspace_bytes.argtypes = [C.POINTER(C.c_int32), C.c_uint32]
    L.vxrt_light_field.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_light_field_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_uint32,
                                        C.c_uint32, C.c_void_p, C.c_void_p]
    L.vxrt_rule_workspace_bytes.restype = C.c_uint64
    L.vxrt_rule_workspace_bytes.argtypes = [C.POINTER(C.c_int32), C.c_void_p]
    L.vxrt_apply_rule.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_apply_rule_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
    L.vxrt_loose_workspace_bytes.restype = C.c_uint64
    L.vxrt_loose_workspace_bytes.argtypes = [C.POINTER(C.c_int32)]
    L.vxrt_loose_step.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_loose_step_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
    L.vxrt_frame_guides.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, f3, f3, f3, f3, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_denoise_workspace_bytes.restype = C.c_uint64
    L.vxrt_denoise_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32]
    L.vxrt_denoise_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(DenoiseParams),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_reproject_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(ReprojectParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_sky_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(SkyParams), C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    L.vxrt_light_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(LightFrameParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_material_field.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(MaterialRulesDesc), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_material_field_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(MaterialRulesDesc),
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_material_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MaterialRulesDesc),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MaterialFrameParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_trace_batch_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FrameStats)]
    for name in EXPORTS:  # every symbol the header declares must resolve
        getattr(L, name)
    _LIB = L
    return L


class VxrtError(RuntimeError):
    pass


def check(rc: int) -> None:
    if rc != 0:
        raise VxrtError(f"vxrt error {rc}: {load().vxrt_last_error().decode()}")
