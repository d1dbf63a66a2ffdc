"""voxelengine_amd -- MI355X-native voxel brickmap ray tracing behind the reference's VoxelRT interface.

Layout: ``csrc/`` hand-written HIP for gfx950 + the C ABI (include/vxrt.h); ``engine`` the host mirror of
``GPUDDA::VoxelRaytracer3D`` / ``GPUDDA::Graphics``; ``sharding`` the screen-strip split and the RCCL gather.
"""
from ._native import (SKY_CLOUDS, SKY_MAX_GLOW_LOG2, SKY_MAX_OCTAVES, SkyParams, MATERIAL_MAX_BANDS, MATERIAL_MAX_TILES, MATERIAL_MAX_TILE_SHIFT, MATERIAL_NO_TILE, MaterialRulesDesc, LOOSE_MAX_STEPS, LOOSE_OPEN, LOOSE_SAND, LOOSE_WALL, LOOSE_WATER, LooseDesc, TRANSFORM_MAX_WORDS, OrientationDesc, RULE_BOX, RULE_MAX_ITERATIONS, RULE_N6, RULE_N18, RULE_N26, RULE_WORLD, RuleDesc, PLACE_MAX_DIM, PLACE_MAX_DIST, PLACE_MAX_PIECES, PLACE_MAX_VOXELS, PLACED_BLOCKED, PLACED_INVALID, PieceDesc, LIGHT_BLOCK, LIGHT_MAX, LIGHT_MAX_EMITTERS, LIGHT_SKY, LF_OCCLUSION, LF_SMOOTH, LOD_MAX_SHIFT, SURF_CAP, SURF_MAX_DIM, SURF_OPEN, VOX_FRAC_BITS, VOX_MAX_COORD, VOX_MAX_DIM, VOX_MAX_TRIANGLES, VOX_SOLID, VOX_SURFACE, DIST_FAR, DIST_MAX_RADIUS, DIST_TO_EMPTY, DIST_TO_SOLID, NAV_AT_GOAL, NAV_MAX_GOALS, NAV_MAX_STEPS, NAV_NONE, NAV_NO_PATH, NAV_OUTSIDE, NAV_TRUNCATED,
                      ISLAND_ANCHOR_FACES, ISLAND_ANCHOR_FLOOR, ISLAND_ANCHOR_X_HI, ISLAND_ANCHOR_X_LO, ISLAND_ANCHOR_Y_HI,
                      ISLAND_ANCHOR_Y_LO, ISLAND_ANCHOR_Z_HI, ISLAND_ANCHOR_Z_LO, BODY_BLOCKED_X, BODY_BLOCKED_Y, BODY_BLOCKED_Z, BODY_INVALID, BODY_MAX_DELTA, BODY_MAX_EXTENT, EDIT_BOX, EDIT_MAX_OPS, EDIT_SPHERE, EMPTY_SLOT, GEN_HASH_HEIGHTFIELD, GEN_INT_TERRAIN, GEN_PERLIN_REF,
                      MAX_STEPS, MODE_DEBUG, MODE_SHADED, STAMP_REPLACE, STAMP_SUBTRACT, STAMP_UNION, EXPORTS, EditOp,
                      EditStats, FrameStats, StampDesc, VxrtError, lib_path, load)
from .engine import (Sky, SkyFrame, SkySummary, MaterialRules, Palette, MaterialField, MaterialSummary, MaterialFrame, MaterialFrameSummary, Loose, LooseResult, LooseSummary, Orientation, TransformedStamp, TransformSummary, Rule, RuleResult, RuleSummary, LitFrame, LightFrameSummary, Reprojected, ReprojectSummary, Piece, Placement, PLACED_DTYPE, DROP_DTYPE, LightField, LightSummary, Downsampled, LodSummary, ExtractedSurface, SurfaceSummary, VoxelizedMesh, VoxelizeSummary, quantize_vertices, DistanceField, DistanceSummary, NavAgent, NavField, NavPaths, NavSummary, nav_move, ISLAND_DTYPE, Body, Context, Islands, IslandSummary, EditBox, EditSphere, GetDirections, RenderOptions, Stamp, compact_rows, grid_is_wide,
                     pack_region, region_words, tile_schedule, unpack_region, world_file_info)

__all__ = ["Context", "RenderOptions", "GetDirections", "compact_rows", "grid_is_wide", "tile_schedule", "world_file_info", "FrameStats",
           "VxrtError", "load",
           "lib_path", "EXPORTS", "EMPTY_SLOT", "MAX_STEPS", "MODE_SHADED", "MODE_DEBUG",
           "GEN_HASH_HEIGHTFIELD", "GEN_PERLIN_REF", "GEN_INT_TERRAIN",
           "EditBox", "EditSphere", "EditOp", "EditStats", "EDIT_BOX", "EDIT_SPHERE", "EDIT_MAX_OPS",
           "Stamp", "StampDesc", "pack_region", "unpack_region", "region_words", "STAMP_REPLACE", "STAMP_UNION",
           "STAMP_SUBTRACT", "Body", "BODY_MAX_EXTENT", "BODY_MAX_DELTA", "BODY_BLOCKED_X", "BODY_BLOCKED_Y",
           "BODY_BLOCKED_Z", "BODY_INVALID", "Islands", "IslandSummary", "ISLAND_DTYPE", "ISLAND_ANCHOR_X_LO",
           "ISLAND_ANCHOR_X_HI", "ISLAND_ANCHOR_Y_LO", "ISLAND_ANCHOR_Y_HI", "ISLAND_ANCHOR_Z_LO", "ISLAND_ANCHOR_Z_HI",
           "ISLAND_ANCHOR_FACES", "ISLAND_ANCHOR_FLOOR", "NavAgent", "NavField", "NavPaths", "NavSummary", "nav_move",
           "NAV_MAX_GOALS", "NAV_NONE", "NAV_MAX_STEPS", "NAV_AT_GOAL", "NAV_NO_PATH", "NAV_TRUNCATED", "NAV_OUTSIDE",
           "DistanceField", "DistanceSummary", "DIST_TO_SOLID", "DIST_TO_EMPTY", "DIST_FAR", "DIST_MAX_RADIUS",
           "VoxelizedMesh", "VoxelizeSummary", "quantize_vertices", "VOX_SURFACE", "VOX_SOLID", "VOX_FRAC_BITS", "VOX_MAX_DIM",
           "VOX_MAX_COORD", "VOX_MAX_TRIANGLES", "ExtractedSurface", "SurfaceSummary", "SURF_CAP", "SURF_OPEN", "SURF_MAX_DIM", "Downsampled", "LodSummary", "LOD_MAX_SHIFT",
           "Reprojected", "ReprojectSummary", "LitFrame", "LightFrameSummary", "LF_SMOOTH", "LF_OCCLUSION",
           "LightField", "LightSummary", "LIGHT_SKY", "LIGHT_BLOCK", "LIGHT_MAX", "LIGHT_MAX_EMITTERS",
           "Rule", "RuleResult", "RuleSummary", "RuleDesc", "RULE_N6", "RULE_N18", "RULE_N26", "RULE_BOX", "RULE_WORLD",
           "RULE_MAX_ITERATIONS", "Loose", "LooseResult", "LooseSummary", "LooseDesc", "LOOSE_SAND", "LOOSE_WATER", "LOOSE_WALL",
           "LOOSE_OPEN", "LOOSE_MAX_STEPS", "Orientation", "OrientationDesc", "TransformedStamp", "TransformSummary", "TRANSFORM_MAX_WORDS",
           "Piece", "Placement", "PieceDesc", "PLACED_DTYPE", "DROP_DTYPE", "PLACE_MAX_PIECES", "PLACE_MAX_DIM", "PLACE_MAX_VOXELS",
           "PLACE_MAX_DIST", "PLACED_BLOCKED", "PLACED_INVALID",
           "MaterialRules", "Palette", "MaterialField", "MaterialSummary", "MaterialFrame", "MaterialFrameSummary", "MaterialRulesDesc",
           "MATERIAL_MAX_BANDS", "MATERIAL_NO_TILE", "MATERIAL_MAX_TILES", "MATERIAL_MAX_TILE_SHIFT",
           "Sky", "SkyFrame", "SkySummary", "SkyParams", "SKY_CLOUDS", "SKY_MAX_GLOW_LOG2", "SKY_MAX_OCTAVES"]
