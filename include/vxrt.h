/*
 * vxrt.h -- C ABI of the MI355X-native voxel brickmap ray tracer (libvxrt.so).
 *
 * Drop-in boundary for the VoxelRT hot path of JoshuaLim007/VoxelEngine.  The
 * reference exposes this path as C++ (namespace GPUDDA); each entry point below
 * names the reference interface it replaces (paths relative to the reference
 * checkout).  A C++ facade with the reference's own names and signatures sits on
 * top of this ABI in include/GPUDDA/ (see INTEGRATION.md).
 *
 * Conventions: every call returns 0 on success or a negative vxrt_status; no
 * exceptions, no exit().  Pointers named d_* are device (HIP) pointers, all
 * others are host pointers.  `stream` is a hipStream_t passed as void* (NULL =
 * HIP's null stream, as in the HIP API).  A context belongs to one device; calls on one
 * context must be serialised by the caller.
 */
#ifndef VXRT_H
#define VXRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VXRT_ABI_VERSION 3
#define VXRT_EMPTY_SLOT 0xFFFFFFFFu
#define VXRT_MAX_STEPS 2048 /* MAX_STEPS, VoxelRT/VolumeRaytracer.cuh:235 */

typedef enum vxrt_status {
    VXRT_OK = 0,
    VXRT_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    VXRT_ERR_HIP = -2,       /* a HIP runtime call failed (see vxrt_last_error) */
    VXRT_ERR_NO_WORLD = -3,  /* render/trace before a world was uploaded or built */
    VXRT_ERR_NOMEM = -4
} vxrt_status;

typedef struct vxrt_ctx vxrt_ctx;

/* ---- lifetime.  Replaces `new GPUDDA::VoxelRaytracer3D(count)` / `delete`
 * (VoxelRT/VolumeRaytracer.cuh:318-334, VoxelApp/main.cu:41,197). */
int vxrt_abi_version(void);
int vxrt_create(int device, vxrt_ctx **out);
int vxrt_destroy(vxrt_ctx *ctx);
/* message of the last failing call on this thread (never NULL) */
const char *vxrt_last_error(void);
int vxrt_synchronize(vxrt_ctx *ctx);
/* kernel implementation used by vxrt_render / vxrt_render_views and vxrt_trace_batch.  Both give identical results.
 *   7 = the product kernels, all on the wave-level tracer of csrc/vxrt_wave2.hpp: k_render_persist2 (persistent
 *       wavefronts, one pixel chain per lane, pixels from a tile queue, the state only the parked phases touch in LDS:
 *       96 VGPRs, 5 waves per SIMD) for every render launch, whatever its size and the world's; for batches
 *       k_trace_batch_persist (a persistent ray queue) from 8 rays per lane of the persistent grid upwards and
 *       k_trace_batch_wave2 (one ray per lane) below that;
 *   4 (default) = 7;
 *   1 = straightforward per-lane loops (k_render, k_trace_batch): the on-device cross-check.
 * Any other value is refused (rounds 1-3 carried further kernels under 0, 2, 3, 5 and 6; profiles/ keeps their
 * measurements). */
int vxrt_set_kernel_variant(vxrt_ctx *ctx, int variant);
/* Test hook of the load guard: on != 0 makes the guard treat the bit tables as if they had been allocated WITHOUT slack
 * (the real allocations are untouched), so that every slack load counts as stray -- the negative control of the test that
 * holds guard_stray_loads at zero. */
int vxrt_debug_guard_pretend_no_slack(vxrt_ctx *ctx, int on);
/* 1 when the library was built with -DVXRT_EXPERIMENTS (development knobs read from the environment; A/B builds) */
int vxrt_has_experiments(void);
/* Size of the persistent kernels' grid, in wavefronts per compute unit at 4 waves per SIMD (default 16 = 4 per SIMD; the
 * kernels, built for 5 waves per SIMD, scale it by 5/4).  For tests that need a small grid (a batch then takes the queue kernel at a few
 * thousand rays) and for occupancy measurements; 0 restores the default. */
int vxrt_set_persistent_waves_per_cu(vxrt_ctx *ctx, int waves_per_cu);

/* ---- world upload.  Replaces VoxelRaytracer3D::UploadVoxelBuffer,
 * ::UploadVoxelBufferDatas, ::UploadVoxelBufferDataBounds and ::SetFactor
 * (VoxelRT/VolumeRaytracer.cu:527-572, VolumeRaytracer.cuh:349).  The three
 * reference tables are handed over as flat host arrays in the reference's own order and copied into HBM (where the
 * library keeps them in an order of its own, x-fastest linear: vxrt_download_world and the brickmap file give the
 * reference's order back):
 *   coarse_bits : one bit per brick cell, tiled-linear order of GetSampleIndex
 *                 (VolumeRaytracer.cuh:107-131), (ncells+31)/32 words
 *   brick_slot  : per cell, index of the brick in `pool` or VXRT_EMPTY_SLOT
 *                 (reference: a VoxelBuffer3D descriptor with its own allocation)
 *   bounds      : per cell 6 floats {min xyz, max xyz}, brick-local inclusive voxel
 *                 extents, empty = {0,0,0,-1,-1,-1} (layout of Bounds3Df)
 *   pool        : nslots bricks of factor^3 bits each, tiled-linear inside the brick */
typedef struct vxrt_world_desc {
    uint32_t struct_size;
    int32_t factor;       /* brick edge: 8, 16 or 32 */
    int32_t cdims[3];     /* coarse cells per axis, each a multiple of 8 */
    uint64_t nslots;
    const uint32_t *coarse_bits;
    const uint32_t *brick_slot;
    const float *bounds;
    const uint32_t *pool;
} vxrt_world_desc;
int vxrt_upload_world(vxrt_ctx *ctx, const vxrt_world_desc *desc);

/* ---- on-device world construction.  Replaces CreateVoxels + PopulateVoxels
 * (VoxelRT/VoxelWorldBuilder.cuh:12-32, .cu:10-35) followed by
 * GenerateLowresVoxelBuffer (VoxelRT/VolumeRaytracer.cuh:379-516), without the
 * dense intermediate: one workgroup per brick evaluates the generator, packs the
 * brick, reduces its extents and sets the coarse bit. */
typedef enum vxrt_generator {
    VXRT_GEN_HASH_HEIGHTFIELD = 0, /* integer-only columns */
    VXRT_GEN_PERLIN_REF = 1,       /* PopulateVoxels' 32-octave Perlin fBm terrain */
    VXRT_GEN_INT_TERRAIN = 2       /* integer-only smooth terrain */
} vxrt_generator;
int vxrt_build_world_procedural(vxrt_ctx *ctx, int generator, int X, int Y, int Z, int factor);

typedef struct vxrt_world_info {
    int32_t factor;
    int32_t cdims[3];
    uint64_t ncells;
    uint64_t nslots;
    uint64_t hbm_bytes; /* bytes resident for the world tables */
} vxrt_world_info;
int vxrt_world_info_get(vxrt_ctx *ctx, vxrt_world_info *out);
/* copy the resident world back in vxrt_world_desc layout; the caller provides host
 * arrays sized from vxrt_world_info_get (pool may be NULL to skip it). */
int vxrt_download_world(vxrt_ctx *ctx, uint32_t *coarse_bits, uint32_t *brick_slot, float *bounds,
                        uint32_t *pool);

/* ---- brickmap file.  The reference rebuilds its world at every start (VoxelApp/main.cu:41-49:
 * CreateVoxels + GenerateLowresVoxelBuffer, minutes at 8k scale on its host threads); a built brickmap can be
 * kept instead.  Layout (little endian): 120-byte header {"VXBRKMAP", u32 version = 2, u32 header bytes,
 * i32 factor, i32 cdims[3], u64 ncells, u64 nslots, u64 bytes of the three streams, u64 word sums of the three
 * streams, u64 sums of the running word sums of the three streams (position-sensitive)}, then the streams as they lie in HBM: coarse_bits (as in vxrt_world_desc), one 8-byte
 * record per cell {u32 pool slot or VXRT_EMPTY_SLOT, u32 extents: min x,y,z then max x,y,z, 5 bits each from bit 0}
 * in the order of coarse_bits, and the pool.  Loading validates sizes, sums and the cell table against the coarse
 * bits, and streams through a 64 MiB staging buffer.  Version 1 files (104-byte header, plain word sums only; written
 * by the first round's builds) are refused: regenerate them with vxrt_save_world.  Shapes: every coarse dimension a
 * positive multiple of 8, at most 65535, with cy * cz < 2^24 and cx * cz * (cy + 2) < 2^32 (32-bit cell indices). */
int vxrt_save_world(vxrt_ctx *ctx, const char *path);
int vxrt_load_world(vxrt_ctx *ctx, const char *path);
/* header of a brickmap file (no GPU needed); hbm_bytes = bytes the three streams will occupy */
int vxrt_world_file_info(const char *path, vxrt_world_info *out);

/* ---- chunk streaming -- an EXTENSION: the reference lists "Chunking" and "Chunk data streaming" as to do
 * (README.md:15,20).  A world whose bricks need not all be resident: the coarse tables of the whole world stay in HBM
 * (128 KiB + 8 MiB for 8192x512x8192), the brick pool is a cache of `pool_capacity_bricks` bricks, and brick data is
 * read from a brickmap file (vxrt_save_world) for the CHUNKS near a focus point only.  A chunk is one 8x8x8 tile of
 * coarse cells -- 512 consecutive records of the file's tiled-linear tables and one contiguous run of bricks, so a
 * chunk arrives with one read, two copies and two small re-ordering launches.  A chunk that is not resident reads as EMPTY space: the kernels do not
 * change, and every frame equals the frame of the world with exactly the resident chunks' bricks (tests hold the HIP
 * frames equal to the oracle on that truncated world).
 *   vxrt_stream_open: replaces the context's world by the (so far empty) streamed world of `path`.  A NULL argument, a
 *     pool_capacity_bricks of 0 or above 0xFFFFFFFF (slots are 32 bits and VXRT_EMPTY_SLOT is none) and a file that
 *     cannot be opened or validated give VXRT_ERR_INVALID before anything changes: the previous world stays.
 *   vxrt_stream_focus: makes every chunk whose box lies within `radius` voxels of `focus` resident, nearest first;
 *     when the pool is full, resident chunks OUTSIDE the radius are evicted, farthest first; chunks inside the radius
 *     that still do not fit stay absent (stats.chunks_missing).  Precisely, in binary32 throughout:
 *     - chunk t = (tx, ty, tz) (index tx + tw * (ty + th * tz), tw = cdims[0] / 8, th = cdims[1] / 8) has the closed box
 *       [8f t, 8f (t + 1)] per axis (f = factor); d^2 = gx^2 + gy^2 + gz^2 summed in that order, g = the focus's gap to
 *       the box on that axis (0 inside); "within the radius" is d^2 <= radius * radius;
 *     - only occupied chunks (those with at least one brick) are considered, in ascending d^2, ties to the lower index;
 *     - a chunk within the radius that is not resident takes the lowest-addressed run of free pool bricks long enough
 *       for it (first fit; bricks freed by evictions are merged with the free runs next to them);
 *     - while no run fits, resident chunks outside the radius are evicted from the far end of the order; each is
 *       scanned at most once per call (the scan does not restart for the next chunk);
 *     - a chunk that still does not fit counts in chunks_missing, and the next chunk is tried;
 *     - a chunk whose read from the file fails (e.g. the file was cut short) ends the call with VXRT_ERR_INVALID at that
 *       chunk: the loads and evictions made before it stay, it is not resident, and stats are not written.  A HIP error
 *       (VXRT_ERR_HIP) ends the call the same way; a chunk whose eviction it interrupts stays resident, and the device
 *       tables of the chunk it stopped at are undefined;
 *     - bytes_read = f^3 / 8 per loaded brick; chunks_loaded / evicted / missing count this call's events.
 *     A NULL ctx or focus, a focus with a non-finite component, or a radius that is negative or NaN give VXRT_ERR_INVALID
 *     and change nothing (radius = +inf is allowed: every occupied chunk is within it).  The call synchronises the device
 *     before it touches the tables, and again before it returns -- on success and on every failure after that point --
 *     so a launch issued after the call on any stream, non-blocking ones included, sees the tables the call left.
 *   vxrt_stream_resident: one byte per chunk (chunk = tile index of the coarse grid), 1 = resident; n_chunks must be the
 *     number of chunks (VXRT_ERR_INVALID otherwise).
 * The coarse tables are validated at open exactly as vxrt_load_world validates them (sizes, position-sensitive sums, slots
 * in cell order, brick extents); brick data read per chunk is NOT checksummed (the file's pool sum covers the whole
 * stream, not its chunks).  vxrt_download_world / vxrt_save_world on a streamed world give the CACHE as it stands: the
 * resident chunks' cells with the cache's own slot numbers, every other cell empty, the pool zero where nothing has been
 * loaded (it is cleared at open) and stale, unreferenced bricks where chunks have been evicted. */
typedef struct vxrt_stream_stats {
    uint64_t chunks_total, chunks_occupied;   /* tiles of the coarse grid; those holding at least one brick */
    uint64_t chunks_resident, bricks_resident;
    uint64_t chunks_loaded, chunks_evicted, chunks_missing;  /* by this call */
    uint64_t bytes_read;                                      /* from the file, by this call */
} vxrt_stream_stats;
int vxrt_stream_open(vxrt_ctx *ctx, const char *path, uint64_t pool_capacity_bricks);
int vxrt_stream_focus(vxrt_ctx *ctx, const float focus[3], float radius, vxrt_stream_stats *stats_or_null);
int vxrt_stream_resident(vxrt_ctx *ctx, uint8_t *flags, uint64_t n_chunks);
int vxrt_stream_close(vxrt_ctx *ctx);

/* ---- voxel editing -- an EXTENSION: the reference lists "Fully modifiable terrain" as to do (README.md:16).  An edit is a
 * list of shape operations applied in order to the voxels of the resident world; afterwards the resident tables are exactly
 * what GenerateLowresVoxelBuffer (VolumeRaytracer.cuh:379-516) builds from the edited dense grid -- coarse bits, per-cell
 * extents and brick contents; only the pool slot numbers may differ -- so every frame and batch afterwards equals the frame
 * of that rebuilt world.
 *   Membership: integer arithmetic only.  A box covers every voxel v with a <= v <= b on each axis; a sphere every voxel
 *     with dx^2 + dy^2 + dz^2 <= r^2 (d = v - a, evaluated without overflow in 64 bits).  Shapes are clipped to the world;
 *     a shape wholly outside it, or an empty box (a > b on some axis), is a no-op.  A voxel takes the value of the LAST op
 *     of the list that covers it, and otherwise keeps its value.
 *   Validation before any change: an unknown kind, a value other than 0 or 1, a negative radius, nonzero b[1] / b[2] on a
 *     sphere, n_ops > VXRT_EDIT_MAX_OPS, or ops == NULL with n_ops > 0 return VXRT_ERR_INVALID; no world gives
 *     VXRT_ERR_NO_WORLD; a streamed world (vxrt_stream_open) gives VXRT_ERR_INVALID (a cache is not edited).
 *   All or nothing: a call that fails -- VXRT_ERR_NOMEM when the pool cannot grow included -- leaves the world unchanged.
 *   Ordering: like vxrt_stream_focus, the call synchronises the device before it touches the tables and returns when the
 *     edit is complete: a launch issued before the call sees the old world, one issued after it the new world.
 *     Accumulation histories (vxrt_render_flags.d_accum) are the caller's to reset.
 *   Brick life cycle: a brick that becomes empty is freed -- its cell reads as empty (VXRT_EMPTY_SLOT, coarse bit 0, the
 *     builder's empty extents), its slot is zeroed and goes on a free list.  A cell that becomes non-empty takes the
 *     lowest free slot, else the next slot past the high-water mark; when the capacity is exhausted the pool grows by
 *     1.5x or more (one copy of the pool; vxrt_edit_reserve grows it ahead of time).  Slot assignment is a host-side scan
 *     in cell order: the same world and the same calls give a byte-identical vxrt_download_world, pool included.
 *   A call that changes no voxel leaves the tables untouched.
 *   vxrt_world_info.nslots is the high-water slot count; vxrt_download_world returns that many bricks, freed ones zero.
 *   vxrt_save_world of a world that an edit has changed writes a COMPACTED pool: live bricks only, numbered in the
 *   tables' tiled cell order as the builders number them, so the file opens with vxrt_stream_open as well.
 *   Precondition: no two cells share a brick slot (true of every world the builders, the loader and the editor make).
 * The cost is proportional to the bricks in the union of the ops' clipped brick boxes (bricks_touched), not to the world;
 * each touched brick needs f^3 / 8 bytes of device scratch for the duration of the call. */
#define VXRT_EDIT_MAX_OPS 1024
typedef enum vxrt_edit_kind { VXRT_EDIT_BOX = 0, VXRT_EDIT_SPHERE = 1 } vxrt_edit_kind;
typedef struct vxrt_edit_op {
    int32_t kind;  /* vxrt_edit_kind */
    int32_t value; /* 1 = set solid, 0 = clear */
    int32_t a[3];  /* BOX: inclusive min voxel; SPHERE: centre voxel */
    int32_t b[3];  /* BOX: inclusive max voxel; SPHERE: b[0] = radius >= 0, b[1] = b[2] = 0 */
} vxrt_edit_op;
typedef struct vxrt_edit_stats {
    uint64_t bricks_touched, bricks_created, bricks_freed; /* by this call */
    uint64_t bricks_live, pool_slots, pool_capacity;       /* after it; pool_slots = high-water slot count = nslots */
} vxrt_edit_stats;
int vxrt_edit_voxels(vxrt_ctx *ctx, const vxrt_edit_op *ops, uint32_t n_ops, vxrt_edit_stats *stats_or_null);
/* grow the pool to at least capacity_bricks now, so that later edits need no copy (never shrinks it) */
int vxrt_edit_reserve(vxrt_ctx *ctx, uint64_t capacity_bricks);

/* ---- region readback and voxel stamps -- an EXTENSION (with the editing above: copy, paste and undo of the resident
 * world).  Copy and paste are a read followed by a stamp; undo is a read of an edit's bounding box before the edit and a
 * VXRT_STAMP_REPLACE stamp of it afterwards.
 * Region bit layout (shared by vxrt_read_region and vxrt_edit_stamps).  A region is a box of dims[0] x dims[1] x dims[2]
 * voxels whose voxel (0,0,0) is world voxel origin.  Row (y, z) of the region is ceil(dims[0] / 32) 32-bit words, rows in
 * order y fastest, then z: voxel (x, y, z) is bit (x & 31) of word (y + dims[1] * z) * ceil(dims[0] / 32) + (x >> 5).
 * Words per region: vxrt_region_words(dims).  Padding bits at the end of a row are written 0 by a read and ignored by a stamp. */
uint64_t vxrt_region_words(const int32_t dims[3]); /* 0 for dims outside 1 <= dims[k], dims[0] * dims[1] * dims[2] <= 2^36 */

/* Asynchronous on `stream`, like vxrt_trace_batch.  Voxels outside the world read 0.  origin may be negative or beyond the
 * world; 1 <= dims[k], dims[0] * dims[1] * dims[2] <= 2^36.  A streamed world gives VXRT_ERR_INVALID (a cache is not read).
 * NULL arguments and bad dims give VXRT_ERR_INVALID, no world VXRT_ERR_NO_WORLD.  The read never loads outside the tables. */
int vxrt_read_region(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t *d_bits, void *stream);
int vxrt_read_region_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t *bits); /* synchronous */

/* Voxel stamps: a list of dense bit volumes (region layout above) written into the resident world in order.
 *   Semantics: let m be the stamp's bit at v - origin.  REPLACE covers every voxel v of the stamp's box and sets it to m;
 *     UNION covers the voxels with m = 1 and sets them to 1; SUBTRACT covers the voxels with m = 1 and clears them.
 *     Stamps are clipped to the world (a stamp wholly outside it is a no-op).  A voxel takes the value the LAST stamp of
 *     the list that covers it gives it, and otherwise keeps its value.
 *   Validation before any change: an unknown mode, nonzero reserved, dims[k] < 1, more than 2^36 voxels, d_bits == NULL,
 *     n_stamps > VXRT_EDIT_MAX_OPS, or stamps == NULL with n_stamps > 0 return VXRT_ERR_INVALID; no world gives
 *     VXRT_ERR_NO_WORLD; a streamed world gives VXRT_ERR_INVALID.
 *   Everything else is vxrt_edit_voxels' contract above: all or nothing (VXRT_ERR_NOMEM on pool growth included), the
 *     device synchronised before and after the call, the brick life cycle, deterministic slot assignment, a call that
 *     changes no voxel writes nothing, vxrt_edit_stats, and the compacting save.
 *   Because the call synchronises the device before it reads any stamp, a stamp may use bits that a vxrt_read_region on
 *     any stream produced just before the call: the undo pattern (read, edit, stamp back) needs no synchronisation of its
 *     own.  The stamp bits must stay valid until the call returns.
 *   Stamps and box / sphere ops are not mixed in one call (two calls, in the order wanted).
 * The cost is proportional to the bricks in the union of the stamps' clipped brick boxes (bricks_touched). */
typedef enum vxrt_stamp_mode { VXRT_STAMP_REPLACE = 0, VXRT_STAMP_UNION = 1, VXRT_STAMP_SUBTRACT = 2 } vxrt_stamp_mode;
typedef struct vxrt_stamp {
    const uint32_t *d_bits;  /* device, region layout above */
    int32_t origin[3];       /* world voxel of the stamp's voxel (0,0,0); may lie partly or wholly outside the world */
    int32_t dims[3];
    int32_t mode;            /* vxrt_stamp_mode */
    int32_t reserved;        /* 0 */
} vxrt_stamp;
int vxrt_edit_stamps(vxrt_ctx *ctx, const vxrt_stamp *stamps, uint32_t n_stamps, vxrt_edit_stats *stats_or_null);

/* ---- box collision queries -- an EXTENSION (with the editing above: bodies kept out of a world that changes).  A body is
 * an axis-aligned box of world voxel coordinates, lo < hi, and a displacement.  Queries read the resident world only.
 *   Voxels.  Voxel v occupies [v, v+1) on each axis.  A box (lo, hi) overlaps the integer range [floor(lo[b]),
 *     ceil(hi[b]) - 1] on axis b: faces that only touch do not overlap.  Voxels outside the world are empty, as they are
 *     for vxrt_read_region.
 *   Move (vxrt_move_boxes).  The body moves axis by axis in `order`, a permutation of {0, 1, 2}; each axis uses the box as
 *     the earlier axes left it.  On axis a, let d = delta[a]; d == 0 (-0 included) does nothing.
 *     d > 0: e = hi[a] + d.  The candidates are the slabs v in [ceil(hi[a]), ceil(e) - 1] crossed with the overlap ranges
 *       of the other two axes.  If a candidate voxel is solid, let F be the least such v: the body is blocked,
 *       lo[a] = lo[a] + ((float)F - hi[a]), then hi[a] = (float)F exactly, and flag bit a is set.  Otherwise
 *       lo[a] = lo[a] + d and hi[a] = e.
 *     d < 0 (the mirror): e = lo[a] + d.  The candidates are [floor(e), floor(lo[a]) - 1].  If one is solid, let G be the
 *       greatest: hi[a] = hi[a] + ((float)(G + 1) - lo[a]), then lo[a] = (float)(G + 1) exactly, and the flag is set.
 *       Otherwise lo[a] = e and hi[a] = hi[a] + d.
 *     Every + / - above is one binary32 operation rounded to nearest, with no contraction.
 *     Consequences: voxels the box already overlaps are ignored, so a body stuck in terrain can move out; a body resting on
 *     a face stays on it (the next step has F = ceil(hi) and is blocked with no move); nothing tunnels, every slab the
 *     leading face sweeps is tested.
 *   Overlap (vxrt_overlap_boxes).  The count is the number of solid voxels in [floor(lo), ceil(hi) - 1] on all three axes;
 *     delta is ignored.
 *   Validity (per body, like the ray validity rule of vxrt_trace_batch).  A body is valid when, on every axis k, every
 *     component is finite, lo[k] < hi[k], hi[k] - lo[k] <= VXRT_BODY_MAX_EXTENT (evaluated in binary32),
 *     |delta[k]| <= VXRT_BODY_MAX_DELTA, and |lo[k]| and |hi[k]| are below 2^24.  An invalid body is returned unchanged
 *     (count 0) with flags VXRT_BODY_INVALID.  The bounds cap the swept slab of one axis at 65 x 65 x 64 voxels.
 *   Call rules (as vxrt_read_region): asynchronous on `stream`.  A NULL ctx, or an `order` that is NULL or not a
 *     permutation, gives VXRT_ERR_INVALID; then n == 0 is a no-op (VXRT_OK); then a NULL required pointer gives
 *     VXRT_ERR_INVALID, no world VXRT_ERR_NO_WORLD, a streamed world VXRT_ERR_INVALID (a cache is not queried).  The
 *     ranges are clipped to the world before any load, so no load falls outside the tables.  Each body's results are its
 *     own: they do not depend on the launch shape, the scheduling or the other bodies.  d_flags_or_null may be NULL.
 * The cost follows the row words the bodies touch: about (cross-section rows) x (swept x words) per axis. */
#define VXRT_BODY_MAX_EXTENT 64 /* voxels, per axis */
#define VXRT_BODY_MAX_DELTA 64  /* voxels, per axis */
#define VXRT_BODY_BLOCKED_X 1u
#define VXRT_BODY_BLOCKED_Y 2u
#define VXRT_BODY_BLOCKED_Z 4u
#define VXRT_BODY_INVALID 8u
typedef struct vxrt_body {
    float lo[3], hi[3], delta[3]; /* 36 bytes; device arrays of n bodies */
} vxrt_body;
/* d_lohi_out: n x 6 floats, lo[3] then hi[3] of each body after the move; d_flags_or_null: n words of VXRT_BODY_* bits */
int vxrt_move_boxes(vxrt_ctx *ctx, const vxrt_body *d_bodies, uint64_t n, const int32_t order[3], float *d_lohi_out,
                    uint32_t *d_flags_or_null, void *stream);
/* d_counts: n words */
int vxrt_overlap_boxes(vxrt_ctx *ctx, const vxrt_body *d_bodies, uint64_t n, uint32_t *d_counts, uint32_t *d_flags_or_null,
                       void *stream);
/* the same on host arrays: copied in and out, synchronous (like vxrt_trace_batch_host) */
int vxrt_move_boxes_host(vxrt_ctx *ctx, const vxrt_body *bodies, uint64_t n, const int32_t order[3], float *lohi_out,
                         uint32_t *flags_or_null);
int vxrt_overlap_boxes_host(vxrt_ctx *ctx, const vxrt_body *bodies, uint64_t n, uint32_t *counts, uint32_t *flags_or_null);

/* ---- floating islands -- an EXTENSION (with the editing above: terrain cut loose by an edit found on the device).  A call
 * looks at one box B = [origin, origin + dims) of world voxels: 1 <= dims[k], dims[0] * dims[1] * dims[2] <= 2^28, and
 * origin[k] + dims[k] <= 2^31 - 1.  B may lie partly outside the world; voxels outside the world are empty, as for
 * vxrt_read_region.
 *   Components.  Two solid voxels of B are connected when they share a face (6-connectivity: edges and corners do not
 *     connect).  Paths never leave B.
 *   Component id.  1 + x + dims[0] * (y + dims[1] * z) of the component's first voxel in that order (x fastest, then y,
 *     then z: the region order of vxrt_read_region).  The id does not depend on the algorithm or the scheduling.
 *   Anchors.  Bits 0-5 of `anchors` are the faces x-lo, x-hi, y-lo, y-hi, z-lo, z-hi of B: a voxel on a set face is an
 *     anchor voxel.  VXRT_ISLAND_ANCHOR_FLOOR makes every voxel at world y = 0 an anchor voxel.  Other bits give
 *     VXRT_ERR_INVALID.  anchors = 0 makes every component an island (plain component labelling, e.g. of a pasted piece).
 *   Island.  A component with no anchor voxel.
 *   Property.  With all six face bits set, every island is a connected piece of the WHOLE world that lies wholly inside B's
 *     interior: every path out of B passes through a face voxel, which would anchor it.  So "edit, then look at the edit's
 *     box grown by a margin of one voxel or more" finds exactly the pieces the edit cut loose there; it is not a heuristic.
 * Outputs:
 *   d_floating: the island voxels in region bit layout (vxrt_region_words(dims) words, padding bits 0).  It is a
 *     VXRT_STAMP_SUBTRACT stamp at `origin` that deletes the islands.
 *   d_labels_or_null: one uint32 per voxel in region order (dims[0] * dims[1] * dims[2] words, no padding): 0 for an empty
 *     voxel, otherwise its component id -- every component, anchored ones included.
 *   d_islands_or_null: one vxrt_island per island in ascending id, at most max_islands rows.  lo / hi are world voxels, hi
 *     exclusive; voxels is the island's voxel count.
 *   d_summary: components, islands (the true count even when the table was cut short) and island_voxels (all islands).
 * Workspace.  d_work holds vxrt_islands_workspace_bytes(dims) bytes, at most 8.5 * voxels + 4 KiB and about 4.6 * voxels
 *   once dims[0] >= 32 (the box's bits, one uint32 parent per voxel and three bits per voxel of root / anchor / prefix
 *   words): 1.2 GiB for a 2^28-voxel box with dims[0] >= 32.  The caller owns it, so calls on different streams share no
 *   hidden scratch; the library allocates nothing per call.
 * Call rules (as vxrt_read_region): asynchronous on `stream`.  A NULL ctx, origin, dims, d_work, d_floating or d_summary,
 *   bad dims or bad anchor bits give VXRT_ERR_INVALID; no world VXRT_ERR_NO_WORLD; a streamed world VXRT_ERR_INVALID (a
 *   cache is not queried).  The call never loads outside the tables.  Results are bit-identical from call to call. */
#define VXRT_ISLAND_ANCHOR_X_LO 0x01u
#define VXRT_ISLAND_ANCHOR_X_HI 0x02u
#define VXRT_ISLAND_ANCHOR_Y_LO 0x04u
#define VXRT_ISLAND_ANCHOR_Y_HI 0x08u
#define VXRT_ISLAND_ANCHOR_Z_LO 0x10u
#define VXRT_ISLAND_ANCHOR_Z_HI 0x20u
#define VXRT_ISLAND_ANCHOR_FACES 0x3Fu
#define VXRT_ISLAND_ANCHOR_FLOOR 0x40u
typedef struct vxrt_island {
    uint32_t id, voxels;  /* component id (above), voxel count */
    int32_t lo[3], hi[3]; /* world voxels, hi exclusive; 32 bytes */
} vxrt_island;
typedef struct vxrt_island_summary {
    uint32_t components, islands, island_voxels;
} vxrt_island_summary;
uint64_t vxrt_islands_workspace_bytes(const int32_t dims[3]); /* 0 for dims outside the contract */
int vxrt_find_islands(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t anchors, void *d_work,
                      uint32_t *d_floating, uint32_t *d_labels_or_null, vxrt_island *d_islands_or_null, uint32_t max_islands,
                      vxrt_island_summary *d_summary, void *stream);
/* the same on host buffers, synchronous; allocates its own workspace (like vxrt_read_region_host) */
int vxrt_find_islands_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t anchors,
                           uint32_t *floating, uint32_t *labels_or_null, vxrt_island *islands_or_null, uint32_t max_islands,
                           vxrt_island_summary *summary);

/* ---- voxel piece queries -- an EXTENSION (with the stamps and islands above: a stamp tested before it is written, loose
 * terrain that falls and lands).  A piece is a rigid dense bit volume in the region layout of vxrt_read_region; a call places
 * up to VXRT_PLACE_MAX_PIECES pieces at n placements against the resident world and only reads it.  Integer arithmetic only.
 *   Piece voxels.  P is the set of voxels p of the piece whose bit is set.  Padding bits at the end of a row are ignored, as a
 *     stamp ignores them.  W(v) is the world's voxel; voxels outside the world are empty, as for every other query.
 *   Overlap at an offset.  For a placement with origin o, axis a and signed distance d let s = sign(d), e the unit vector of
 *     axis a and ov(j) = |{p in P : W(o + p + s * j * e)}|.
 *   overlap = ov(0).
 *   travel = s * k, k the largest integer in [0, |d|] with ov(j) = 0 for every 1 <= j <= k: every step is tested, nothing
 *     tunnels, and ov(0) plays no part, so a piece that starts inside terrain can move out.  Equivalently k = min(|d|, the
 *     least clearance of a piece voxel along the axis).
 *   Blocked.  If k < |d|, flags = VXRT_PLACED_BLOCKED and contact = ov(k + 1), the voxels that stop the piece; otherwise
 *     contact = 0.  d = 0 is a pure fit test.  A piece with no set bit travels the whole distance with overlap 0.
 *   Validity (per placement, like the body validity rule).  A placement is valid when 0 <= piece < n_pieces, axis is 0, 1 or
 *     2, |dist| <= VXRT_PLACE_MAX_DIST and |origin[k]| <= 2^30 on every axis.  An invalid placement returns
 *     {0, 0, 0, VXRT_PLACED_INVALID}.
 * Call rules, checked in this order: a NULL ctx gives VXRT_ERR_INVALID; so do n_pieces outside 1 .. 64, a NULL `pieces`, a
 *   piece with NULL bits, nonzero `reserved`, a dim outside 1 .. VXRT_PLACE_MAX_DIM or more than VXRT_PLACE_MAX_VOXELS voxels;
 *   n = 0 is then a no-op (VXRT_OK); NULL placements or results give VXRT_ERR_INVALID; no world VXRT_ERR_NO_WORLD; a streamed
 *   world VXRT_ERR_INVALID.  `pieces` is a HOST array whose descriptors travel by value; the bits they name stay on the
 *   device.  Asynchronous on `stream`.  The library allocates nothing per call and needs no workspace: d_results holds the
 *   accumulators while the call runs.  The call never loads outside the tables, or outside vxrt_region_words(dims) words of
 *   a piece.  Every result is its placement's own: it does not depend on the batch, the launch shape or the scheduling, and
 *   is bit-identical from call to call.  (All placements of a call share one launch shape, sized by the piece with the most
 *   rows: batch big pieces apart from small ones for speed, not for results.) */
#define VXRT_PLACE_MAX_PIECES 64
#define VXRT_PLACE_MAX_DIM 1024          /* per axis */
#define VXRT_PLACE_MAX_VOXELS (1u << 24) /* dims[0] * dims[1] * dims[2] */
#define VXRT_PLACE_MAX_DIST 4096
#define VXRT_PLACED_BLOCKED 1u
#define VXRT_PLACED_INVALID 2u
typedef struct vxrt_piece {
    const uint32_t *d_bits; /* device, region layout: vxrt_region_words(dims) words */
    int32_t dims[3];
    int32_t reserved;       /* 0 */
} vxrt_piece;
typedef struct vxrt_placement {
    int32_t piece, origin[3], axis, dist; /* 24 bytes */
} vxrt_placement;
typedef struct vxrt_placed {
    uint32_t overlap;
    int32_t travel;
    uint32_t contact, flags; /* 16 bytes */
} vxrt_placed;
int vxrt_place_pieces(vxrt_ctx *ctx, const vxrt_piece *pieces /* HOST array */, uint32_t n_pieces,
                      const vxrt_placement *d_placements, uint64_t n, vxrt_placed *d_results, void *stream);
/* the same with the pieces' bits (the pointers in `pieces`), the placements and the results in host memory: copied in and
 * out, synchronous; allocates its own device buffers (like vxrt_read_region_host) */
int vxrt_place_pieces_host(vxrt_ctx *ctx, const vxrt_piece *pieces, uint32_t n_pieces, const vxrt_placement *placements,
                           uint64_t n, vxrt_placed *results);

/* ---- stamp orientations -- an EXTENSION (with the stamps and pieces above: a clipboard that turns).  Everything in the
 * region layout of vxrt_read_region -- a region read, a stamp, a piece, a voxelized mesh, the island bits, the result of a
 * rule or of a downsampling -- can be rotated and mirrored on the device into one of its 48 orientations.
 *   Orientation.  A signed axis permutation: destination axis k runs along source axis axis[k], and against it when bit k
 *     of `flip` is set.  For source dims sd the destination dims are dd[k] = sd[axis[k]], and source voxel p lands at q with
 *     q[k] = flip bit k ? sd[axis[k]] - 1 - p[axis[k]] : p[axis[k]]; equivalently dst(q) = src(p) for the p this inverts to.
 *     axis must be a permutation of {0, 1, 2} and the bits of flip above 2 must be 0: all 48 such orientations are valid.
 *     The 24 with sign(axis) * (-1)^popcount(flip) = +1 are rotations, the others mirror.
 *   Helpers.  Host only, integer only, no context and no device (like vxrt_get_directions); each returns VXRT_ERR_INVALID for
 *     a NULL argument or an invalid orientation, else VXRT_OK.  `out` may be an input.
 *     vxrt_orientation_rotation: `quarter_turns` right-handed quarter turns about `axis` (0, 1, 2; anything else is invalid):
 *       one turn takes axis a + 1 onto axis a + 2 (mod 3), so one turn about z is axis = {1, 0, 2}, flip = 1:
 *       q = (sd[1] - 1 - p[1], p[0], p[2]).  Any turn count is taken mod 4, negative ones included.
 *     vxrt_orientation_compose: a first, then b: out.axis[k] = a.axis[b.axis[k]],
 *       out.flip bit k = b.flip bit k XOR a.flip bit b.axis[k].
 *     vxrt_orientation_inverse: compose(o, inverse(o)) is the identity {0, 1, 2}, 0.
 *     vxrt_orientation_dims and vxrt_orientation_voxel: dd and q of the rule above (a pivot, or where to paste); the dims and
 *       the voxel are not checked.
 *     vxrt_orientation_is_rotation: 1 or 0, VXRT_ERR_INVALID (negative) for an invalid orientation or NULL.
 *   vxrt_transform_stamp.  d_src holds vxrt_region_words(src_dims) words; padding bits at the end of a source row are
 *     ignored, as a stamp ignores them.  Every one of the vxrt_region_words(dd) words of d_dst is written exactly once, its
 *     padding bits 0, and nothing behind them is touched: the result is directly a stamp, a piece or a mask.
 *     d_summary_or_null: voxels = the set voxels of the source (padding ignored) = those of the destination; set_min /
 *     set_max = their inclusive bounds in DESTINATION coordinates, INT32_MAX / INT32_MIN on every axis when there is none (as
 *     vxrt_rule_summary).  The summary is accumulated in d_summary itself with integer atomics after an initialisation on
 *     the stream; with NULL the bits are the same.
 *   Limits.  src_dims within vxrt_region_words' contract; vxrt_region_words(src_dims) and vxrt_region_words(dd) both at
 *     most VXRT_TRANSFORM_MAX_WORDS = 2^31 (a row of one voxel still takes a word, so dd can need 32 times the source's
 *     words).  Word indices then fit 32 bits; byte offsets do not, and the library forms addresses in 64 bits.
 *     d_src and d_dst must not overlap: overlapping ranges are refused.
 *   Call rules.  The call needs a context but no world: it never returns VXRT_ERR_NO_WORLD and works with a streamed world
 *     resident, because it reads no table.  Asynchronous on `stream`; no host synchronisation, no allocation per call and no
 *     workspace, so it can be captured.  The result is a function of the arguments alone and bit-identical from call to
 *     call.  Checked in this order, each VXRT_ERR_INVALID: a NULL ctx; a NULL d_src, src_dims, o or d_dst; an invalid
 *     orientation; bad dims; the word caps; overlap.  A refused call enqueues and writes nothing.
 *   vxrt_transform_stamp_host takes host buffers (src in; dst and the summary out), allocates its own device buffers and is
 *     synchronous; its ranges may not overlap either.
 * The cost is one pass: every source word is read once and every destination word written once.  Orientations that keep x
 *   (axis[0] == 0, 16 of them) move whole rows; the 32 that move x transpose 32 x 32 bit tiles through LDS. */
#define VXRT_TRANSFORM_MAX_WORDS (1ull << 31)
typedef struct vxrt_orientation {
    int32_t axis[3]; /* a permutation of {0,1,2}: destination axis k runs along source axis axis[k] */
    uint32_t flip;   /* bit k: destination axis k runs against the source axis; bits above 2 must be 0 */
} vxrt_orientation;
typedef struct vxrt_transform_summary {
    uint64_t voxels;                /* set voxels of the source (padding ignored) = set voxels of the destination */
    int32_t set_min[3], set_max[3]; /* inclusive bounds of the set voxels in DESTINATION coordinates;
                                       INT32_MAX / INT32_MIN on every axis when there is none (as vxrt_rule_summary) */
} vxrt_transform_summary;           /* 32 bytes */
int vxrt_orientation_rotation(int axis, int quarter_turns, vxrt_orientation *out);
int vxrt_orientation_compose(const vxrt_orientation *a, const vxrt_orientation *b, vxrt_orientation *out);
int vxrt_orientation_inverse(const vxrt_orientation *o, vxrt_orientation *out);
int vxrt_orientation_dims(const vxrt_orientation *o, const int32_t src_dims[3], int32_t dst_dims[3]);
int vxrt_orientation_voxel(const vxrt_orientation *o, const int32_t src_dims[3], const int32_t p[3], int32_t q[3]);
int vxrt_orientation_is_rotation(const vxrt_orientation *o);
int vxrt_transform_stamp(vxrt_ctx *ctx, const uint32_t *d_src, const int32_t src_dims[3], const vxrt_orientation *o,
                         uint32_t *d_dst, vxrt_transform_summary *d_summary_or_null, void *stream);
int vxrt_transform_stamp_host(vxrt_ctx *ctx, const uint32_t *src, const int32_t src_dims[3], const vxrt_orientation *o,
                              uint32_t *dst, vxrt_transform_summary *summary_or_null);

/* ---- navigation fields -- an EXTENSION (with the editing above: where a body can walk, and which way is the goal).  A call
 * looks at one box B = [origin, origin + dims) of world cells, with the limits of vxrt_find_islands: 1 <= dims[k],
 * dims[0] * dims[1] * dims[2] <= 2^28, origin[k] + dims[k] <= 2^31 - 1.  Voxels outside the world are empty.
 *   Agent.  vxrt_nav_agent: 1 <= width <= 8, 1 <= height <= 32, 0 <= climb <= 8, 0 <= drop <= 32.  A cell c = (x, y, z) is
 *     the agent's minimum corner; the agent occupies A(c) = [x, x+width) x [y, y+height) x [z, z+width).
 *     free(c): every voxel of A(c) is empty (this reads the world, not only B).
 *     supported(c): some voxel of [x, x+width) x {y-1} x [z, z+width) is solid.
 *     A node is a cell of B that is free and supported.
 *   Moves.  From node c, one candidate per direction d in the order (+x, -x, +z, -z) and per dy in the order (0, +1, ..,
 *     +climb, -1, .., -drop); the target is t = c + d + (0, dy, 0).  The move is valid when t is a node and
 *       dy = 0: nothing more;
 *       dy > 0: free(c + (0, k, 0)) for k = 1 .. dy (the agent rises in place, then steps over);
 *       dy < 0: free(c + d + (0, k, 0)) for k = dy+1 .. 0 (the agent steps over the edge, then falls).
 *     Every cell these conditions name lies in B when t does.  Moves are not symmetric: a cliff is dropped, not climbed.
 *     Move code = 1 + (direction index) * (1 + climb + drop) + (index of dy in its order): 1 .. 164.
 *   Goals.  Up to VXRT_NAV_MAX_GOALS cells (3 int32 each).  A goal that is not a node is ignored and counted.
 *     dist(c) is the least number of valid moves from node c to any goal node; above max_dist (1 <= max_dist <= 2^24), or
 *     with no path, c is unreachable.  next(c) is 0 for a goal node; for another reachable node, the code of the first
 *     valid move in code order whose target t has dist(t) = dist(c) - 1; VXRT_NAV_NONE for non-nodes and unreachable nodes.
 *     dist and next are functions of the world, B, the agent, the goals and max_dist alone, not of the algorithm or the
 *     scheduling.
 * Outputs of vxrt_nav_field, all in region order (x fastest, then y, then z, as vxrt_read_region):
 *   d_walkable: the node bits in region bit layout (vxrt_region_words(dims) words, padding bits 0).
 *   d_next: one byte per cell (required).
 *   d_dist_or_null: one uint32 per cell, 0xFFFFFFFF for unreachable cells and non-nodes.
 *   d_summary: nodes; goals_used (goal entries that are nodes, repeats counted) and goals_ignored (the others); reached
 *     (reachable nodes, goal nodes included); max_dist_found; levels = max_dist_found + 1, or 0 when no goal is used;
 *     tiles_total, the BFS tiles of B (32 x 16 x 16 cells: ceil(dims[0] / 32) * ceil(dims[1] / 16) * ceil(dims[2] / 16));
 *     tile_visits, the (level, tile) pairs the call processed (the work follows the frontier: a level visits the tiles
 *     next to the cells the level before reached, not all of B).
 * Workspace.  d_work holds vxrt_nav_workspace_bytes(dims, agent) bytes, 0 outside the contract.  With W = width,
 *   H = height, r(n) = n rounded up to a multiple of 64, wb = ceil(dims[0] / 32), wh = ceil((dims[0] + W - 1) / 32),
 *   hy = dims[1] + H, hz = dims[2] + W - 1, nb = wb * dims[1] * dims[2], n = dims[0] * dims[1] * dims[2] and T = tiles_total:
 *     bytes = 4 * (r(wh * hy * hz) + r(wb * hy * hz) + 2 * r(wb * dims[1] * hz) + 4 * r(nb) + r(n) + r(6 * T) + 64)
 *   (the halo's bits, the erosion passes, free / visited / two frontier planes, the distances, the tile lists): a little over
 *   4 bytes per cell.  The caller owns it; the library allocates nothing per call.
 * Call rules.  vxrt_nav_field runs on `stream`, after the work already queued there, and RETURNS WHEN THE FIELD IS COMPLETE:
 *   the number of BFS levels depends on the data, so the host reads a termination flag from the device every few levels
 *   (a stream synchronisation).  vxrt_nav_paths is asynchronous on `stream`.  A NULL ctx, origin, dims, agent, d_work,
 *   d_walkable, d_next or d_summary, d_goals NULL with n_goals > 0, bad dims, agent or max_dist, or n_goals >
 *   VXRT_NAV_MAX_GOALS give VXRT_ERR_INVALID; no world VXRT_ERR_NO_WORLD; a streamed world VXRT_ERR_INVALID (a cache is not
 *   queried).  n_goals = 0 gives a field with no goal: walkable is filled, every cell is unreachable.  The call never loads
 *   outside the tables.  Results are bit-identical from call to call.
 * Paths (vxrt_nav_paths).  The input is a field description (origin, dims, agent, d_next of a vxrt_nav_field call) and n
 *   start cells (3 int32 each, world cells).  For each start the kernel follows the next codes for at most max_steps moves
 *   (max_steps <= 65535); it reads no world data, only the codes.  d_cells_or_null: n x (max_steps + 1) x 3 int32, the
 *   cells visited from the start on, each path padded with its last cell; d_lengths: the moves made; d_status:
 *   VXRT_NAV_AT_GOAL (the path ends on a goal node), VXRT_NAV_NO_PATH (the start is not a reachable node; also a code
 *   that no vxrt_nav_field call writes there, met on the way), VXRT_NAV_TRUNCATED (max_steps moves made, no goal yet) or
 *   VXRT_NAV_OUTSIDE (the start is not in B).  A NULL ctx, field, field d_next, d_starts, d_lengths or d_status, bad
 *   dims or agent, or max_steps > 65535 give VXRT_ERR_INVALID; then n == 0 is a no-op.  No world is needed.
 * vxrt_nav_field_host copies goals in and the outputs out (host buffers, the same sizes), allocates its own workspace and
 *   is synchronous. */
#define VXRT_NAV_MAX_GOALS 4096
#define VXRT_NAV_NONE 0xFFu
#define VXRT_NAV_MAX_STEPS 65535
#define VXRT_NAV_AT_GOAL 0u
#define VXRT_NAV_NO_PATH 1u
#define VXRT_NAV_TRUNCATED 2u
#define VXRT_NAV_OUTSIDE 3u
typedef struct vxrt_nav_agent {
    int32_t width, height, climb, drop;
} vxrt_nav_agent;
typedef struct vxrt_nav_summary {
    uint32_t nodes, goals_used, goals_ignored, reached, max_dist_found, levels, tiles_total, tile_visits;
} vxrt_nav_summary;
typedef struct vxrt_nav_field_desc {
    int32_t origin[3], dims[3];
    vxrt_nav_agent agent;
    const uint8_t *d_next; /* the d_next of a vxrt_nav_field call on this box and agent */
} vxrt_nav_field_desc;
uint64_t vxrt_nav_workspace_bytes(const int32_t dims[3], const vxrt_nav_agent *agent); /* 0 outside the contract */
int vxrt_nav_field(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_nav_agent *agent,
                   const int32_t *d_goals, uint32_t n_goals, uint32_t max_dist, void *d_work, uint32_t *d_walkable,
                   uint8_t *d_next, uint32_t *d_dist_or_null, vxrt_nav_summary *d_summary, void *stream);
int vxrt_nav_paths(vxrt_ctx *ctx, const vxrt_nav_field_desc *field, const int32_t *d_starts, uint64_t n, uint32_t max_steps,
                   int32_t *d_cells_or_null, uint32_t *d_lengths, uint32_t *d_status, void *stream);
/* the field on host buffers, synchronous; allocates its own workspace */
int vxrt_nav_field_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_nav_agent *agent,
                        const int32_t *goals, uint32_t n_goals, uint32_t max_dist, uint32_t *walkable, uint8_t *next,
                        uint32_t *dist_or_null, vxrt_nav_summary *summary);

/* ---- exact distance fields -- an EXTENSION (with the editing above: how far the nearest surface is, recomputed on the
 * device after every edit).  A call looks at one box B = [origin, origin + dims) of world voxels and a radius R.
 *   Targets.  VXRT_DIST_TO_SOLID: the solid voxels of the world.  VXRT_DIST_TO_EMPTY: the empty voxels; voxels outside the
 *     world are empty (as for vxrt_read_region), so they are targets too.  Targets are voxels of the WHOLE world, not only
 *     of B: the call reads the halo [origin - R, origin + dims + R).
 *   Value.  For voxel v of B, d2(v) = min over targets t of (vx-tx)^2 + (vy-ty)^2 + (vz-tz)^2: the squared Euclidean
 *     distance between voxel indices, an integer; 0 for a target.  The output is d2(v) when d2(v) <= R^2 and VXRT_DIST_FAR
 *     otherwise.  The field is exact, not a chamfer or jump-flood approximation: a target with d2 <= R^2 is at most R away
 *     on every axis, so it lies in the halo, and the three separable sweeps (x, then y, then z, each over offsets -R .. R)
 *     take the minimum over every target of the halo; a partial sum above R^2 can only end above R^2.  The value does not
 *     depend on the algorithm or the scheduling.
 *   Limits.  1 <= R <= VXRT_DIST_MAX_RADIUS (R^2 = 65025 < VXRT_DIST_FAR, so the field is one uint16_t per voxel);
 *     1 <= dims[k]; dims[0] * dims[1] * dims[2] <= 2^28; the halo box (dims[k] + 2R per axis) within vxrt_read_region's
 *     2^36 voxels; origin[k] - R >= -2^31 and origin[k] + dims[k] + R <= 2^31 - 1.
 * Outputs:
 *   d_dist2: one uint16_t per voxel in region order (x fastest, then y, then z, no padding, as d_labels of
 *     vxrt_find_islands).
 *   d_summary: zero (voxels of B that are targets), near (values 1 .. R^2), far (VXRT_DIST_FAR), max_d2 (the largest value
 *     that is not FAR, 0 when there is none), sum_d2 (the sum of the values that are not FAR: a checksum for callers that
 *     do not want the whole field back).
 * Workspace.  d_work holds vxrt_distance_workspace_bytes(dims, radius) bytes, 0 outside the limits on dims and radius.  With
 *   r(n) = n rounded up to a multiple of 256, h[k] = dims[k] + 2R, wh = ceil(h[0] / 32) and T[k] = ceil(dims[k] / 64):
 *     bytes = r(4 * wh * h[1] * h[2]) + r(2 * dims[0] * dims[1] * h[2]) + r(wh * ceil(h[1] / 8) * ceil(h[2] / 8))
 *             + r(T[0] * T[1] * T[2])
 *   (the halo's bits, the uint16 field after the y sweep over every halo slice, one occupancy byte per 32 x 8 x 8 halo
 *   voxels, one byte per 64^3 tile of B): 2 * (1 + 2R / dims[2]) bytes per voxel and the halo's bits.  The caller owns it; the
 *   library allocates nothing per call.
 * Call rules (as vxrt_find_islands): asynchronous on `stream`.  Checked in this order: a NULL ctx, origin, dims, d_work,
 *   d_dist2 or d_summary; the radius; the dims and the halo box; the origin; the mode -- each VXRT_ERR_INVALID; then no
 *   world VXRT_ERR_NO_WORLD; a streamed world VXRT_ERR_INVALID (a cache is not queried).  A refused call writes nothing.
 *   The call never loads outside the tables.  Results are bit-identical from call to call.
 * vxrt_distance_field_host copies the outputs to host buffers (the same sizes), allocates its own workspace and is
 *   synchronous. */
#define VXRT_DIST_MAX_RADIUS 255
#define VXRT_DIST_FAR 0xFFFFu
typedef enum vxrt_dist_mode { VXRT_DIST_TO_SOLID = 0, VXRT_DIST_TO_EMPTY = 1 } vxrt_dist_mode;
typedef struct vxrt_distance_summary {
    uint32_t zero, near, far, max_d2;
    uint64_t sum_d2;
} vxrt_distance_summary;
uint64_t vxrt_distance_workspace_bytes(const int32_t dims[3], uint32_t radius); /* 0 outside the contract */
int vxrt_distance_field(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t radius, int32_t mode,
                        void *d_work, uint16_t *d_dist2, vxrt_distance_summary *d_summary, void *stream);
/* the same on host buffers, synchronous; allocates its own workspace */
int vxrt_distance_field_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t radius, int32_t mode,
                             uint16_t *dist2, vxrt_distance_summary *summary);

/* ---- mesh voxelization -- an EXTENSION (with the stamps above: a triangle mesh turned into a stamp on the device).  The
 * call reads no world: it works with none resident and with a streamed one.
 *   Coordinates.  Fixed point, VXRT_VOX_FRAC_BITS = 8: 256 units per voxel.  d_vertices is int32[n_vertices][3] in the frame
 *     of the output region; region voxel (i, j, k) is the cube [256 i, 256 (i+1)] x [256 j, 256 (j+1)] x [256 k, 256 (k+1)]
 *     and its centre is (256 i + 128, 256 j + 128, 256 k + 128).  d_triangles is uint32[n_triangles][3] vertex indices.  The
 *     mesh may extend outside the region; it is clipped to it.
 *   Limits.  1 <= dims[k] <= VXRT_VOX_MAX_DIM = 1024; every vertex coordinate that a triangle uses lies in
 *     [-2^18, 2^18] (VXRT_VOX_MAX_COORD); n_triangles <= VXRT_VOX_MAX_TRIANGLES = 2^24.  Hence the arithmetic bound:
 *     coordinate differences stay below 2^20, cross-product components below 2^40 and a plane value n . (p - v0) below
 *     2^62, so every quantity below is exact in int64.
 *   Validity (per triangle, like the body validity rule).  A triangle is INVALID when one of its indices is >= n_vertices
 *     or one of its vertices has a coordinate outside the range; DEGENERATE when it is valid and its normal
 *     n = (v1 - v0) x (v2 - v0) is the zero vector.  Both kinds contribute nothing and are counted.
 *   VXRT_VOX_SURFACE.  Voxel (i, j, k) is set if and only if some valid, non-degenerate triangle, as a closed set,
 *     intersects the voxel's closed cube; touching counts.  Decided exactly by the 13-axis separating-axis test in integers
 *     (the 3 cube axes, the normal, the 9 products edge x cube axis); a pair is separated only on a strict inequality.
 *   VXRT_VOX_SOLID.  Voxel (i, j, k) is set if and only if an odd number of valid, non-degenerate triangles are CROSSED by
 *     the ray from its centre c toward +x.  Triangle T is crossed when
 *     (a) T covers (cy, cz) in the yz projection: never when n.x == 0; otherwise T is oriented so that n.x > 0 (v1 and v2
 *         swapped when n.x < 0), and for each directed edge a -> b, with the inward normal (ey, ez) = (-(b.z - a.z), b.y - a.y)
 *         and E = ey (cy - a.y) + ez (cz - a.z): E > 0, or E == 0 and (ey > 0 or (ey == 0 and ez > 0)) -- the top-left rule;
 *     (b) the plane meets the ray strictly beyond the centre: sign(n.x) * (n . (c - v0)) < 0.
 *     This is the test of the point (cx + eta, cy + eps, cz + eps^2), 0 < eps << eta << 1: for a closed mesh the parity is
 *     the inside test of a generic point; a shared edge or vertex is never counted twice or missed; a box mesh [a, b) fills
 *     exactly the centres a <= c < b (voxel v occupies [v, v+1)).  Equivalent form per (T, j, k): with x* the plane's x at
 *     (cy, cz), m = clamp(ceil((x* - 128) / 256), 0, dims[0]) and T toggles voxels 0 .. m-1 of row (j, k).  A triangle beyond
 *     the region's +x face is crossed like any other (the part of a closed mesh that sticks out closes the parity).
 *   The result does not depend on triangle order, vertex order within a triangle, winding or scheduling.
 *   modes: a non-zero subset of {VXRT_VOX_SURFACE, VXRT_VOX_SOLID}; the output is the OR of the chosen fields.
 * Outputs:
 *   d_bits: vxrt_read_region's layout, vxrt_region_words(dims) words, padding bits 0: a vxrt_stamp's d_bits as it is.
 *   d_summary: set (bits set in the output); surface, solid (bits of each chosen field, 0 for one not chosen); triangles
 *     (n_triangles); invalid; degenerate; outside (valid triangles whose closed bounding box misses the closed region box
 *     [0, 256 dims]).
 * Workspace.  d_work holds vxrt_voxelize_workspace_bytes(dims, n_triangles) bytes, 0 outside the limits.  With r(n) = n
 *   rounded up to a multiple of 256 and W = ceil(dims[0] / 32) * dims[1] * dims[2]:
 *     bytes = r(4 * W) + r(4 * n_triangles) + r(8 * ceil(n_triangles / 256)) + 256
 *   (the solid field's toggle bits, one item offset per triangle, one per group of 256 triangles, the counters).  The caller
 *   owns it; the library allocates nothing per call and never synchronises with the host inside the call.
 * Call rules (as vxrt_distance_field): asynchronous on `stream`.  Checked in this order: a NULL ctx, dims, d_work, d_bits
 *   or d_summary; modes outside {1, 2, 3}; the dims; n_triangles above the limit; d_vertices or d_triangles NULL with
 *   n_triangles > 0 -- each VXRT_ERR_INVALID.  n_triangles == 0 is valid: zeroed bits and summary.  A refused call writes
 *   nothing.  Results are bit-identical from call to call.
 * vxrt_voxelize_mesh_host takes host buffers, allocates its own workspace and is synchronous.
 * The cost follows the voxels near the triangles (blocks of 64 x 8 x 8 voxels and their rows are culled by the same exact
 * test before any voxel is tested), the yz area of the triangles (solid) and one pass over the output. */
#define VXRT_VOX_FRAC_BITS 8
#define VXRT_VOX_MAX_DIM 1024
#define VXRT_VOX_MAX_COORD (1 << 18)
#define VXRT_VOX_MAX_TRIANGLES (1u << 24)
#define VXRT_VOX_SURFACE 1
#define VXRT_VOX_SOLID 2
typedef struct vxrt_voxelize_summary {
    uint32_t set, surface, solid, triangles, invalid, degenerate, outside, reserved;
} vxrt_voxelize_summary;
uint64_t vxrt_voxelize_workspace_bytes(const int32_t dims[3], uint32_t n_triangles); /* 0 outside the contract */
int vxrt_voxelize_mesh(vxrt_ctx *ctx, const int32_t *d_vertices, uint32_t n_vertices, const uint32_t *d_triangles,
                       uint32_t n_triangles, const int32_t dims[3], int32_t modes, void *d_work, uint32_t *d_bits,
                       vxrt_voxelize_summary *d_summary, void *stream);
int vxrt_voxelize_mesh_host(vxrt_ctx *ctx, const int32_t *vertices, uint32_t n_vertices, const uint32_t *triangles,
                            uint32_t n_triangles, const int32_t dims[3], int32_t modes, uint32_t *bits,
                            vxrt_voxelize_summary *summary);

/* ---- surface extraction -- an EXTENSION (the opposite direction of mesh voxelization: the surface of a box of the
 * resident world as quads and, optionally, triangles in vxrt_voxelize_mesh's input format).
 *   Box.  One call looks at one box B = [origin, origin + dims) of world voxels; voxels outside the world are empty, as for
 *     vxrt_read_region.
 *   Limits.  1 <= dims[k] <= VXRT_SURF_MAX_DIM = 1024 (output coordinates at 256 units per voxel stay within
 *     VXRT_VOX_MAX_COORD); dims[0] * dims[1] * dims[2] <= 2^28; origin[k] - 1 >= -2^31 and origin[k] + dims[k] + 1 <= 2^31 - 1.
 *   Directions.  d = 0 .. 5 means -x, +x, -y, +y, -z, +z; the axis of d is a = d / 2; the in-plane axes (u, v) are the other
 *     two in ascending order: (y, z) for x, (x, z) for y, (x, y) for z.
 *   Faces.  Voxel p of B has a face in direction d when p is solid and its neighbour p + d is empty.
 *   mode.  VXRT_SURF_CAP (0): neighbours outside B count as empty; the mesh is a closed surface.  VXRT_SURF_OPEN (1):
 *     neighbours outside B are the world's own voxels, so that chunk meshes tile without interior walls.  Outside the world
 *     is empty in both modes.
 *   Quads ("run-stack" merging).  For direction d and slice s (the coordinate of p along a, in box coordinates) the faces
 *     form a 2-D mask over (u, v).  A RUN of row v is a maximal interval [u, u + w) of set bits of that row.  A QUAD
 *     (u, v, w, h) is a maximal set of consecutive rows v .. v + h - 1 that each have [u, u + w) as a run: row v - 1 and row
 *     v + h do not have that run.  Every face lies in exactly one quad.  Whether a quad exists is a local property of the
 *     mask: the result does not depend on a scan order or on scheduling.
 *   Output order.  Ascending (d, s, v, u).
 *   Quad record.  vxrt_quad, 8 bytes: pos = x | y << 10 | z << 20, the lowest box-relative voxel of the quad;
 *     ext = (w - 1) | (h - 1) << 10 | d << 20.
 *   Triangles (optional; d_vertices and d_triangles both NULL or both given).  Quad i yields vertices 4 i .. 4 i + 3 (int32
 *     xyz, 256 units per voxel, in the box's frame): the corners (u, v), (u + w, v), (u + w, v + h), (u, v + h) on the plane
 *     a = 256 (s + (d & 1)); and triangles 2 i and 2 i + 1 (uint32 indices), split along the diagonal from corner 0 to
 *     corner 2 and wound so that (v1 - v0) x (v2 - v0) is a positive multiple of the outward direction d: (0, 1, 2), (0, 2, 3)
 *     for d = 1, 2, 5 and (0, 2, 1), (0, 3, 2) for d = 0, 3, 4.  Vertices are not welded.  The CAP mesh voxelized with
 *     VXRT_VOX_SOLID into `dims` gives B's bits again.  With triangles at most 2^30 quads are written (their indices fit
 *     uint32): a larger capacity_quads counts as 2^30.
 *   Capacity.  Only the first min(quads, capacity_quads) records in the output order are written, with their vertices and
 *     triangles; nothing past them is touched.  capacity_quads == 0 with NULL outputs is a valid counting call.
 * Outputs:
 *   d_quads: capacity_quads records; d_vertices: 12 int32 per quad; d_triangles: 6 uint32 per quad.
 *   d_summary: solid (solid voxels of B); faces; quads (the full count, whatever the capacity); written; faces_dir[6];
 *     quads_dir[6].
 * Workspace.  d_work holds vxrt_surface_workspace_bytes(dims) bytes, 0 outside the limits.  With r(n) = n rounded up to a
 *   multiple of 256, H = ceil((dims[0] + 2) / 32) * (dims[1] + 2) * (dims[2] + 2) and R = 2 * dims[2] * (dims[0] + 2 * dims[1]):
 *     bytes = r(4 * H) + r(4 * R) + r(4 * ceil(R / 256))
 *   (the bits of B grown by one voxel, one count per row of a mask, one per group of 256 rows).  The caller owns it; the
 *   library allocates nothing per call and never synchronises with the host inside the call.
 * Call rules (as vxrt_distance_field): asynchronous on `stream`.  Checked in this order: a NULL ctx, origin, dims, d_work or
 *   d_summary; the mode; the dims; the origin; d_quads NULL with capacity_quads > 0; only one of d_vertices and d_triangles
 *   given -- each VXRT_ERR_INVALID; then no world: VXRT_ERR_NO_WORLD; then a streamed world: VXRT_ERR_INVALID.  A refused call
 *   writes nothing.  The call never loads outside the tables.  Results are bit-identical from call to call.
 * vxrt_extract_surface_host takes host buffers, allocates its own workspace and is synchronous.
 * The cost is one region read of the grown box, two passes over its face bits (a count and an emit, a scan of the row
 * counts between them) and the records written. */
#define VXRT_SURF_MAX_DIM 1024
#define VXRT_SURF_CAP 0
#define VXRT_SURF_OPEN 1
typedef struct vxrt_quad {
    uint32_t pos, ext;
} vxrt_quad;
typedef struct vxrt_surface_summary {
    uint32_t solid, faces, quads, written;
    uint32_t faces_dir[6], quads_dir[6];
} vxrt_surface_summary;
uint64_t vxrt_surface_workspace_bytes(const int32_t dims[3]); /* 0 outside the contract */
int vxrt_extract_surface(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], int32_t mode, void *d_work,
                         vxrt_quad *d_quads, uint32_t capacity_quads, int32_t *d_vertices, uint32_t *d_triangles,
                         vxrt_surface_summary *d_summary, void *stream);
int vxrt_extract_surface_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], int32_t mode, vxrt_quad *quads,
                              uint32_t capacity_quads, int32_t *vertices, uint32_t *triangles, vxrt_surface_summary *summary);

/* ---- occupancy LOD -- an EXTENSION (the reference's to-do item "LOD, further chunks with lower voxel resolution": a box
 * of the resident world reduced by 2^shift per axis on the device, as bits and as counts).  One call looks at one box of
 * CELLS, with f = 1 << shift and 1 <= shift <= VXRT_LOD_MAX_SHIFT = 5.
 *   Cell.  Cell C = (X, Y, Z), 0 <= C[k] < dims[k], covers the f^3 world voxels origin + f * C + [0, f)^3.  `origin` is any
 *     int32 triple: it need not be a multiple of f, and may be negative or beyond the world.  Voxels outside the world are
 *     empty, as for vxrt_read_region.
 *   Count.  c(C) is the number of solid voxels of the cell, 0 .. f^3.  f^3 <= 32768, so a count is one uint16_t.
 *   Bit.  c(C) >= threshold, with 1 <= threshold <= f^3.  threshold = 1 is ANY: it is conservative (nothing thin
 *     disappears, a ray that misses the coarse world misses the fine one), the choice for ray tracing and collision
 *     proxies.  threshold = f^3 is ALL; threshold = f^3 / 2 is the majority.
 *   Limits.  dims[k] >= 1.  The source box S[k] = f * dims[k] has S[0] * S[1] * S[2] <= 2^32 voxels: every S[k] stays within
 *     int32 and the workspace at most 512 MiB; a larger volume is tiled by the caller, in z slabs for instance.
 *     origin[k] >= -2^31 and origin[k] + S[k] <= 2^31 - 1.
 * Outputs:
 *   d_bits: the cell bits in vxrt_read_region's layout for `dims` (vxrt_region_words(dims) words, padding bits 0): a
 *     vxrt_stamp's d_bits as it is.
 *   d_counts_or_null: one uint16_t per cell in region order (x fastest, then y, then z, no padding, as d_dist2).
 *   d_summary: solid (the sum of all counts: the solid voxels of the source box), set (cells with c >= threshold), empty
 *     (c == 0), full (c == f^3), mixed (the rest), max_count, reserved (0).
 *   The result does not depend on the scheduling: two calls are bit-identical.
 * Workspace.  d_work holds vxrt_lod_workspace_bytes(dims, shift) bytes, 0 outside the limits on dims and shift.  With
 *   r(n) = n rounded up to a multiple of 256 and S[k] = dims[k] << shift:
 *     bytes = r(4 * ceil(S[0] / 32) * S[1] * S[2])
 *   (the bits of the source box, vxrt_region_words(S) words; the reduction needs no further section).  The caller owns it;
 *   the library allocates nothing per call and never synchronises with the host inside the call.
 * Call rules (as vxrt_distance_field): asynchronous on `stream`.  Checked in this order: a NULL ctx, origin, dims, d_work,
 *   d_bits or d_summary; the shift; the threshold; the dims and the source box; the origin -- each VXRT_ERR_INVALID; then no
 *   world: VXRT_ERR_NO_WORLD; then a streamed world: VXRT_ERR_INVALID (a cache is not queried).  A refused call writes
 *   nothing.  The call never loads outside the tables.
 * vxrt_downsample_region_host takes host buffers (the same sizes; counts_or_null may be NULL), allocates its own workspace
 *   and is synchronous.
 * The cost is one region read of the source box and one pass over its words: every source word is loaded once and counted
 *   with word operations, never voxel by voxel. */
#define VXRT_LOD_MAX_SHIFT 5
typedef struct vxrt_lod_summary {
    uint64_t solid;
    uint32_t set, empty, full, mixed, max_count, reserved;
} vxrt_lod_summary;
uint64_t vxrt_lod_workspace_bytes(const int32_t dims[3], uint32_t shift); /* 0 outside the contract */
int vxrt_downsample_region(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t shift, uint32_t threshold,
                           void *d_work, uint32_t *d_bits, uint16_t *d_counts_or_null, vxrt_lod_summary *d_summary,
                           void *stream);
int vxrt_downsample_region_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], uint32_t shift,
                                uint32_t threshold, uint32_t *bits, uint16_t *counts_or_null, vxrt_lod_summary *summary);

/* ---- voxel light fields -- an EXTENSION (the reference's to-do item "Proper indirect lighting" in its cheap, exact,
 * edit-friendly form: flood-fill light, recomputed on the device for the box an edit touched).  A call looks at one box
 * B = [origin, origin + dims) of world voxels.  +y is up, as for vxrt_nav_field.  Voxels outside the world are empty, as for
 * vxrt_read_region.
 *   Levels and channels.  A level is 0 .. VXRT_LIGHT_MAX = 15.  `channels` is a non-empty subset of VXRT_LIGHT_SKY = 1 and
 *     VXRT_LIGHT_BLOCK = 2.
 *   Transparent and solid.  An empty voxel carries light.  A solid voxel has level 0 in both channels and passes none on.
 *   Sky sources.  Voxel v is EXPOSED when v is empty and every voxel (v.x, y', v.z) with y' > v.y is empty -- over the WHOLE
 *     world, not only B or its halo: everything at or above the world's top is exposed, and so is everything beside the
 *     world in x or z.  An exposed voxel is a sky source of level 15.
 *   Block sources.  d_emitters is n_emitters x int32[4] (x, y, z, level), at most VXRT_LIGHT_MAX_EMITTERS = 65536 entries.
 *     Every entry falls in exactly one class: INVALID (level outside 1 .. 15); FAR (valid level, the voxel outside the
 *     halo box below: it cannot reach B, and its voxel is not looked at); SOLID (valid level, in the halo box, a solid voxel:
 *     ignored); USED (valid level, in the halo box, an empty voxel: a block source of that level).  Several used entries on
 *     one voxel give it the largest of their levels.
 *   Value.  Per channel, with g(s, v) the length of the shortest 6-connected path from s to v through empty voxels
 *     (infinite when there is none): level(v) = max(0, max over sources s of level(s) - g(s, v)) for an empty v, and 0 for
 *     a solid v.  Equivalently the least fixed point of level(v) = max(source(v), max over the six neighbours n of
 *     level(n) - 1) on the empty voxels.  The value is a function of the world, B and the emitters alone: it does not depend
 *     on the algorithm or the scheduling.
 *   Halo.  H = VXRT_LIGHT_MAX - 1 = 14.  A level >= 1 at v needs a source s with level(s) - g(s, v) >= 1, so g(s, v) <= 14:
 *     s is at most 14 steps away, and every voxel of such a path is within 14 steps of v, so the path never leaves the box
 *     of +-14 around v.  For v in B that box lies in the halo box [origin - 14, origin + dims + 14): the call reads the
 *     halo box and, for the sky channel (whether a halo voxel is exposed depends on its whole column), the columns above
 *     it up to the world's top.  The levels computed for halo voxels outside B may be too low; they are not output.
 *   Limits.  1 <= dims[k]; dims[0] * dims[1] * dims[2] <= 2^28; the halo box (dims[k] + 28 per axis) within
 *     vxrt_read_region's 2^36 voxels; origin[k] - 14 >= -2^31 and origin[k] + dims[k] + 14 <= 2^31 - 1;
 *     n_emitters <= VXRT_LIGHT_MAX_EMITTERS.
 * Outputs:
 *   d_levels: one byte per voxel of B in region order (x fastest, then y, then z, no padding, as d_dist2):
 *     (sky << 4) | block.  The nibble of a channel that is not requested is 0.
 *   d_summary: solid (solid voxels of B); exposed (exposed voxels of B; 0 without the sky channel); hist_sky[16] and
 *     hist_block[16] (the EMPTY voxels of B by level; a channel that is not requested has all of them in entry 0, so each
 *     histogram always sums to the empty voxels of B); sum_sky and sum_block (the sum of the channel's levels over B: a
 *     checksum for callers that do not want the whole field back); emitters_used, emitters_solid, emitters_far,
 *     emitters_invalid (entries per class; they sum to n_emitters).  Without the block channel d_emitters is not read and
 *     all four counts are 0, whatever n_emitters is (only the check n_emitters <= VXRT_LIGHT_MAX_EMITTERS is made).
 * Workspace.  d_work holds vxrt_light_workspace_bytes(dims, channels) bytes, 0 outside the limits on dims and channels.  It
 *   depends on dims and channels only, never on the world.  With r(n) = n rounded up to a multiple of 256,
 *   h[k] = dims[k] + 28, wh = ceil(h[0] / 32), P = 4 * wh * h[1] * h[2] (one bit plane of the halo box), n = the number of
 *   channels requested, s = 1 with the sky channel and b = 1 with the block channel (else 0):
 *     bytes = r(P) * (1 + 6 * n) + s * r(4 * wh * h[2]) + b * 8 * VXRT_LIGHT_MAX_EMITTERS
 *   (the halo's empty bits; per channel two planes for the level sets in turn and four for the bit-sliced level; the
 *   "blocked above" bit per (x, z) of the halo, reduced from the columns above it in slabs of 8 rows straight from the
 *   tables -- the columns are never materialised; one 8-byte record per emitter).  The caller owns it; the library
 *   allocates nothing per call.
 * Call rules (as vxrt_distance_field): asynchronous on `stream`; the launches follow from the arguments and the world's
 *   height alone (14 rounds whatever the world holds), and the call never synchronises with the host.  Checked in this
 *   order: a NULL ctx, origin, dims, d_work, d_levels or d_summary; the channels; n_emitters above the limit, or d_emitters
 *   NULL with n_emitters > 0 and the block channel set; the dims and the halo box; the origin -- each VXRT_ERR_INVALID;
 *   then no world: VXRT_ERR_NO_WORLD; then a streamed world: VXRT_ERR_INVALID (a cache is not queried).  A refused call
 *   writes nothing.  The call never loads outside the tables.  Two calls are bit-identical.
 * vxrt_light_field_host takes host buffers (emitters in; levels and summary out, the same sizes), allocates its own
 *   workspace and is synchronous.
 * The cost is one region read of the halo box, the columns above it for the sky channel, and 14 rounds of word
 *   operations over six bit planes per channel; no voxel is visited on its own before the bytes are written.  After an
 *   edit a caller relights the edit's box grown by 14 on every axis: no level outside it can have changed. */
#define VXRT_LIGHT_MAX 15
#define VXRT_LIGHT_SKY 1
#define VXRT_LIGHT_BLOCK 2
#define VXRT_LIGHT_MAX_EMITTERS 65536u
typedef struct vxrt_light_summary {
    uint32_t solid, exposed;
    uint32_t hist_sky[16], hist_block[16];
    uint64_t sum_sky, sum_block;
    uint32_t emitters_used, emitters_solid, emitters_far, emitters_invalid;
} vxrt_light_summary;
uint64_t vxrt_light_workspace_bytes(const int32_t dims[3], uint32_t channels); /* 0 outside the contract */
int vxrt_light_field(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const int32_t *d_emitters,
                     uint32_t n_emitters, uint32_t channels, void *d_work, uint8_t *d_levels, vxrt_light_summary *d_summary,
                     void *stream);
int vxrt_light_field_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const int32_t *emitters,
                          uint32_t n_emitters, uint32_t channels, uint8_t *levels, vxrt_light_summary *summary);

/* ---- voxel rules -- an EXTENSION (the reference's to-do item "Better landscape generation" in its classic cheap form, a
 * 3-D cellular automaton, and with the editing above the smooth / grow / erode brush): every voxel of a box replaced by a
 * function of itself and of how many of its neighbours are solid, a few times over, without leaving the bit-packed form.  A
 * call looks at one box B = [origin, origin + dims) of world voxels and changes nothing: its result is a stamp.
 *   Neighbourhoods.  For an offset d != 0 with d in {-1, 0, 1}^3: VXRT_RULE_N6 holds the offsets with |d|_1 = 1, VXRT_RULE_N18
 *     those with |d|_1 <= 2, VXRT_RULE_N26 all 26.  N = 6, 18, 26 is their number.
 *   Step.  For a world state W (one bit per voxel), S(W)(v) = bit c of `survive` if W(v) = 1, else bit c of `born`, where
 *     c = the sum over the neighbourhood's offsets d of W(v + d).  A voxel outside the world has the constant value
 *     `outside` (0: empty, as for vxrt_read_region; 1: solid) in every W_i and is never changed.
 *   Free voxels.  F is the set a step may change.
 *     VXRT_RULE_BOX: F = B intersected with the world and, with a mask, only the voxels whose mask bit is 1.  The mask is in
 *       B's region layout, vxrt_region_words(dims) words; its padding bits are ignored.  Everything else is frozen at W_0:
 *       the rule runs on the box alone, and n iterations give exactly what n calls of one iteration would give, each
 *       followed by a VXRT_STAMP_REPLACE stamp of its result.  The halo is h = 1.
 *     VXRT_RULE_WORLD: F = the world.  B is a window into the result of running the rule n times on the whole world, so
 *       tiles computed from the same W_0 meet without seams.  A value in B after n steps depends on W_0 within Chebyshev
 *       distance n, so the halo is h = iterations.  A mask is refused.
 *   Iteration.  W_0 = the resident world; W_i+1(v) = S(W_i)(v) for v in F, and W_i(v) otherwise, for i = 0 .. n - 1 with
 *     n = `iterations`.  The result is a function of the world, the arguments and the mask alone: it does not depend on the
 *     scheduling, and two calls are bit-identical.
 *   Limits.  1 <= dims[k]; dims[0] * dims[1] * dims[2] <= 2^28; the halo box (dims[k] + 2 h per axis) within
 *     vxrt_read_region's 2^36 voxels; origin[k] - h >= -2^31 and origin[k] + dims[k] + h <= 2^31 - 1;
 *     1 <= iterations <= VXRT_RULE_MAX_ITERATIONS = 16.
 * Outputs:
 *   d_bits: W_n over B in region layout (vxrt_region_words(dims) words), padding bits 0.  Voxels of B outside the world are 0
 *     whatever `outside` says.  It is directly usable as a VXRT_STAMP_REPLACE stamp at `origin`.
 *   d_summary: over the world voxels of B only.  solid_before = the voxels with W_0 = 1, solid_after those with W_n = 1;
 *     born = the voxels that are 0 in W_0 and 1 in W_n, died those that are 1 in W_0 and 0 in W_n, so
 *     solid_after = solid_before + born - died; changed_last = the voxels with W_n != W_n-1 (0: a fixed point was reached);
 *     changed_min / changed_max = the inclusive bounding box, in world coordinates, of the voxels with W_n != W_0, and
 *     INT32_MAX / INT32_MIN on every axis when there is none: the box to stamp, to relight (grown by 14) and after which to
 *     reset a frame history.  reserved_ is 0.  Integer sums and integer min / max only.
 * Workspace.  d_work holds vxrt_rule_workspace_bytes(dims, rule) bytes, 0 outside the limits on dims and the rule's fields.
 *   It depends on dims and the rule only, never on the world.  With r(n) = n rounded up to a multiple of 256, h the halo,
 *   hd[k] = dims[k] + 2 h, wh = ceil(hd[0] / 32) and P = 4 * wh * hd[1] * hd[2] (one bit plane of the halo box):
 *     bytes = 4 * r(P)
 *   (W_0, F and the two planes the rounds write in turn).  The caller owns it; the library allocates nothing per call.
 * Call rules (as vxrt_light_field): asynchronous on `stream`; the launches follow from the arguments alone (`iterations`
 *   rounds whatever the world holds), the call never synchronises with the host and can be captured.  Checked in this order:
 *   a NULL ctx, origin, dims, rule, d_work, d_bits or d_summary; the rule's struct_size; neighbours; bits of born or survive
 *   above N; iterations; scope; outside; a nonzero reserved_; a mask given with VXRT_RULE_WORLD; the dims and the halo box;
 *   the origin -- each VXRT_ERR_INVALID; then no world: VXRT_ERR_NO_WORLD; then a streamed world: VXRT_ERR_INVALID (a cache is
 *   not queried).  A refused call enqueues and writes nothing.  The call never loads outside the tables.
 * vxrt_apply_rule_host takes host buffers (the mask in; bits and summary out, the same sizes), allocates its own workspace
 *   and is synchronous.
 * The cost is one region read of the halo box and `iterations` rounds of word operations over its bit planes: per output
 *   word 27 plane words read and about 200 word operations, no voxel visited on its own.  A world-sized pass is made of
 *   VXRT_RULE_WORLD calls on tiles, all made before the first of their stamps is written. */
#define VXRT_RULE_MAX_ITERATIONS 16
typedef enum vxrt_rule_neighbours { VXRT_RULE_N6 = 0, VXRT_RULE_N18 = 1, VXRT_RULE_N26 = 2 } vxrt_rule_neighbours;
typedef enum vxrt_rule_scope { VXRT_RULE_BOX = 0, VXRT_RULE_WORLD = 1 } vxrt_rule_scope;
typedef struct vxrt_rule {
    uint32_t struct_size;
    int32_t neighbours;  /* vxrt_rule_neighbours; N = 6, 18, 26 */
    uint32_t born;       /* bit c: an empty voxel with c solid neighbours becomes solid; bits above N must be 0 */
    uint32_t survive;    /* bit c: a solid voxel with c solid neighbours stays solid; bits above N must be 0 */
    int32_t iterations;  /* 1 .. VXRT_RULE_MAX_ITERATIONS */
    int32_t scope;       /* vxrt_rule_scope */
    int32_t outside;     /* 0: voxels outside the world count as empty (as vxrt_read_region); 1: as solid */
    int32_t reserved_;   /* 0 */
} vxrt_rule;
typedef struct vxrt_rule_summary {
    uint32_t solid_before, solid_after, born, died, changed_last, reserved_;
    int32_t changed_min[3], changed_max[3];
} vxrt_rule_summary;
uint64_t vxrt_rule_workspace_bytes(const int32_t dims[3], const vxrt_rule *rule); /* 0 outside the contract */
int vxrt_apply_rule(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_rule *rule,
                    const uint32_t *d_mask_or_null, void *d_work, uint32_t *d_bits, vxrt_rule_summary *d_summary, void *stream);
int vxrt_apply_rule_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_rule *rule,
                         const uint32_t *mask_or_null, uint32_t *bits, vxrt_rule_summary *summary);

/* ---- loose voxels -- an EXTENSION: a layer of sand or water that falls, slides and spreads over the world's solids.  The
 * neighbour-count rules above have no "down"; this is the directional step rule that conserves mass.  A call looks at one
 * box B = [origin, origin + dims) of world voxels and changes nothing in the world.
 *   Loose layer.  The loose material is a second bit volume that the caller owns, in B's region layout
 *     (vxrt_region_words(dims) words; its padding bits are ignored).  The call advances it by `steps` steps against the
 *     world's solids and returns the new layer in the same layout: directly usable as a stamp at `origin`.
 *   Gravity is -y (the world is Y-up).  Every coordinate below is a world coordinate, so a result does not depend on where
 *     the box was cut.
 *   Sets.  W = the world's solid bits.  Live = B intersected with the world.  Under VXRT_LOOSE_WALL a voxel outside Live is
 *     BLOCKED.  Under VXRT_LOOSE_OPEN a voxel outside Live is blocked where W is 1 and a SINK where W is 0 (outside the world
 *     W reads 0, as in vxrt_read_region): material that moves into a sink disappears.  A Live voxel is blocked where W is 1.
 *     For a layer L, free(v) = v is not blocked and v is not in L; a sink is always free.  L_start = the input's valid bits
 *     that are Live and not solid: bits on solids, outside the world or in padding are dropped.
 *   Step t = phase + i (mod 2^32), i = 0 .. steps - 1.  A step is two passes for sand and three for water, strictly one
 *     after the other, each evaluated on the layer the pass before left; all moves of a pass are simultaneous.
 *     1. FALL.  Every v in L with free(v - e_y) moves to v - e_y.
 *     2. SLIDE.  a = t & 1 (0: the x axis, 1: the z axis).  For v = (x, y, z), c = z when a = 0 and c = x when a = 1,
 *        s = (c + y + (t >> 1)) & 1, and d(v) = +e_a if s = 0, else -e_a.  Every v in L that is resting (not free(v - e_y))
 *        with free(v + d) and free(v + d - e_y) moves to v + d - e_y.
 *     3. SPREAD (VXRT_LOOSE_WATER only).  With the same d(v), every resting v in L with free(v + d) moves to v + d.
 *     A mover whose target is a sink is removed.  Within a pass two movers never share a target: two sources of one target
 *     lie on one axis line with the same y and the same c, hence have the same sign, and a target is one voxel away from its
 *     source along that sign.  The direction varies with position parity and is not one global rotation, under which a lone
 *     voxel and a lone hole both walk a closed four-cell loop and water never finds a pit.  Water here spreads and fills, but
 *     it is not a pressure solver: it does not level perfectly over isolated one-cell pits.
 *     Sand reaches a fixed point: fell_last = slid_last = 0 is "at rest".  Water at rest in a basin still moves its top layer
 *     sideways; fell_last = slid_last = 0 is its "level" signal.  A step offers every voxel one direction only, so one quiet
 *     step is a signal, not a proof: the layer is a fixed point once four steps running, one of each phase & 3, move nothing.
 *   Steps across calls.  `steps` steps in one call equal `steps` calls of one step, each fed the previous output with `phase`
 *     advanced by one.  Only phase & 3 matters.
 *   Limits.  1 <= dims[k]; dims[0] * dims[1] * dims[2] <= 2^28; the halo box (dims[k] + 2 per axis) within vxrt_read_region's
 *     2^36 voxels; origin[k] - 1 >= -2^31 and origin[k] + dims[k] + 1 <= 2^31 - 1; 1 <= steps <= VXRT_LOOSE_MAX_STEPS = 64.
 * Outputs:
 *   d_loose_out: L_n over B in region layout, padding bits 0.  It may be exactly d_loose_in (a call in place); no other
 *     overlap is allowed.
 *   d_summary: loose_in = the input's valid bits over B (padding excluded); loose_start = |L_start|, loose_after = |L_n|, so
 *     dropped = loose_in - loose_start and drained = loose_start - loose_after; fell_last, slid_last, spread_last = the movers
 *     of each pass of the last step (spread_last is 0 for sand); changed_min / changed_max = the inclusive world box of the
 *     voxels where L_n differs from the input's valid bits, INT32_MAX / INT32_MIN on every axis when there is none.
 * Workspace.  d_work holds vxrt_loose_workspace_bytes(dims) bytes, 0 outside the limits on dims.  With r(n) = n rounded up to a
 *   multiple of 256, hd[k] = dims[k] + 2, wh = ceil(hd[0] / 32) and P = 4 * wh * hd[1] * hd[2] (one bit plane of the halo box,
 *   as for vxrt_apply_rule with h = 1):
 *     bytes = 4 * r(P)
 *   (blocked, live and the two planes the passes write in turn).  The caller owns it; the library allocates nothing per call.
 * Call rules (as vxrt_apply_rule): asynchronous on `stream`; the launches follow from the arguments alone (one region read, one
 *   set-up, `steps` times two or three passes, one output), the call never synchronises with the host and can be captured.
 *   Checked in this order: a NULL ctx, origin, dims, params, d_loose_in, d_work, d_loose_out or d_summary; struct_size;
 *   material; steps; edge; a nonzero reserved_; the dims and the halo box; the origin -- each VXRT_ERR_INVALID; then no world:
 *   VXRT_ERR_NO_WORLD; then a streamed world: VXRT_ERR_INVALID.  A refused call enqueues and writes nothing.
 * vxrt_loose_step_host takes host buffers (the layer in and out, the summary out), allocates its own workspace and is
 *   synchronous. */
#define VXRT_LOOSE_MAX_STEPS 64
typedef enum vxrt_loose_material { VXRT_LOOSE_SAND = 0, VXRT_LOOSE_WATER = 1 } vxrt_loose_material;
typedef enum vxrt_loose_edge { VXRT_LOOSE_WALL = 0, VXRT_LOOSE_OPEN = 1 } vxrt_loose_edge;
typedef struct vxrt_loose {
    uint32_t struct_size;
    int32_t material;  /* vxrt_loose_material */
    int32_t steps;     /* 1 .. VXRT_LOOSE_MAX_STEPS */
    int32_t edge;      /* vxrt_loose_edge */
    uint32_t phase;    /* the number t of the call's first step */
    int32_t reserved_[3]; /* 0 */
} vxrt_loose;
typedef struct vxrt_loose_summary {
    uint32_t loose_in, loose_start, loose_after, fell_last, slid_last, spread_last;
    int32_t changed_min[3], changed_max[3];
} vxrt_loose_summary;
uint64_t vxrt_loose_workspace_bytes(const int32_t dims[3]); /* 0 outside the contract */
int vxrt_loose_step(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_loose *params,
                    const uint32_t *d_loose_in, void *d_work, uint32_t *d_loose_out, vxrt_loose_summary *d_summary, void *stream);
int vxrt_loose_step_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_loose *params,
                         const uint32_t *loose_in, uint32_t *loose_out, vxrt_loose_summary *summary);

/* ---- camera / lighting state.  Replaces Graphics::SetEnvironment, ::SetFOV,
 * ::SetOrthoWindowSize, ::GetDirections (VoxelRT/Renderer.cu:27-42,278-303). */
int vxrt_set_environment(vxrt_ctx *ctx, const float light_dir[3], const float light_color[3],
                         const float ambient[3]);
int vxrt_set_fov(vxrt_ctx *ctx, float fov_degrees);
int vxrt_set_ortho_window_size(vxrt_ctx *ctx, float size_x, float size_y);
void vxrt_get_directions(const float euler[3], float fwd[3], float up[3], float right[3]);

/* ---- per-frame render.  Replaces Graphics::RenderScreen + kernel screenDispatch
 * (VoxelRT/Renderer.cu:179-328).  The compile-time switches of the reference are
 * run-time flags here. */
typedef enum vxrt_mode { VXRT_MODE_SHADED = 0, VXRT_MODE_DEBUG = 1 } vxrt_mode;

typedef struct vxrt_frame_stats {
    uint64_t primary_rays, shadow_rays, bounce_rays, primary_hits;
    uint64_t coarse_probes; /* Nc: in-range coarse cell probes */
    uint64_t brick_entries; /* Nb */
    uint64_t fine_probes;   /* Nf: in-range brick cell probes */
    uint64_t dbg[13];       /* wave-loop diagnostics of collect_stats launches, summed over waves: [0] iterations,
                               [1] walking lanes over those iterations, [2] end-of-walk / [3] tight-box / [4] ray-finished
                               phase executions, [5..7] lanes those executions served (same order); persistent kernel
                               only: [8] wave lifetime in 100 MHz ticks, [9] iterations after the tile queue ran dry, [10] ticks inside
                               the ray-finished phase, [11] ticks inside the box and end-of-walk phases, [12] shadow rays launched
                               from the end-of-walk phase (primary hits that went on without parking) */
    /* Load guard of collect_stats launches (product kernels).  The tracer lets a lane that has just stepped out of a grid
     * issue one more occupancy load before it stops; the library allocates slack around both bit tables for it.  Counted
     * per load: beyond a table but inside its allocation (expected, > 0 on ordinary frames), and outside everything
     * addressable (must be 0: a world path that forgot the slack would show up here, not as a fault in a user's frame). */
    uint64_t guard_slack_loads, guard_stray_loads;
} vxrt_frame_stats;

typedef struct vxrt_render_flags {
    uint32_t struct_size;
    int32_t mode;            /* vxrt_mode; DEBUG = `#define DEBUG_VIEW` (Renderer.cu:4) */
    int32_t checkerboard;    /* ENABLE_CHECKERBOARD_RENDER (Renderer.cu:5) */
    int32_t shadow;          /* 1 = shadow ray of Renderer.cu:97-102 enabled */
    int32_t bounce_samples;  /* `samples` of Renderer.cu:123 */
    int32_t bounce_all_hits; /* 0 = reference gate `lDot == 0` (Renderer.cu:121); 1 = every hit pixel */
    int32_t bounce_depth;    /* <= 1 (default): the reference's one occlusion ray per sample.  2: EXTENSION beyond the
                                reference (BASELINE config 5): a sample ray that hits spawns one more 8-step ray from
                                its hit point, built like the first (outward normal there, seed + 500); a miss of
                                that ray adds 0.5 to the sample sum */
    int32_t ortho;           /* `#define ORTHO` (Renderer.cuh:13) */
    int64_t frame_number;    /* >= 0: value the kernel sees as FrameNumber; < 0: the context's own
                                counter with the reference's post-copy increment (Renderer.cu:310,322) */
    /* multi-GPU strip sharding: rows are cut into strips of `strip_rows`; strip s belongs to
     * shard s % strip_count.  strip_count <= 1 renders the whole frame. */
    int32_t strip_rows, strip_count, strip_index;
    int32_t compact;         /* 1: d_fb (and AOVs) hold only this shard's strips, packed in order: frame row y is row
                                (y / strip_rows / strip_count) * strip_rows + y % strip_rows of vxrt_compact_rows rows;
                                0: the buffers are full-size and the shard's rows sit at their frame rows.  Either way a
                                launch writes the shard's pixels only (under checkerboard: those the frame's launch
                                writes) and every other entry of d_fb, the AOVs and d_accum keeps its contents; a shard
                                that owns no strip writes nothing, counts nothing and succeeds.  Bad strip arguments with
                                strip_count > 1 (strip_rows <= 0, strip_index outside 0 .. strip_count - 1) and frames of
                                more than 65535 rows are refused with VXRT_ERR_INVALID before anything is written */
    int32_t collect_stats;   /* 1: also count probes (the STATS instantiation of the same kernel); rays are always counted */
    int32_t tile_schedule;   /* persistent kernel: 1 (default) = hand out the rows of 8x8 pixel tiles expected-longest
                                first (ranked per frame on the host by the elevation of the row's centre ray in a
                                Y-up world); 0 = row-major.  Scheduling only: results do not depend on it */
    float *d_color_aov;      /* optional W*H*3 float colour handed to the pixel store, or NULL */
    int64_t *d_hit_aov;      /* optional W*H primary hit voxel index (x + X*(y + Y*z)) or -1, or NULL */
    const uint32_t *d_tile_order; /* optional caller-made hand-out order, overrides tile_schedule: a permutation of
                                0 .. ceil(W/8)*ceil(rows/8)-1 (tile = tx + ty*ceil(W/8), rows = the launch grid's), or NULL */
    void *stream;
    /* Temporal accumulation of the stochastic occlusion term -- an EXTENSION: the reference lists "denoise, temporal
     * accumulation" as to do (README.md:19).  d_accum: W*H*4 floats per pixel {sum r, g, b of the pre-tonemap colour, frames
     * in the history} (compact shards: their own rows), or NULL = off.  For every shaded hit pixel the colour of
     * calculateColor (Renderer.cu:90-168) is added to the history and the MEAN is tonemapped and stored; the first frame of
     * a history (accum_reset != 0, or frames == 0) stores the colour itself.  Miss pixels, the debug view and the overlays
     * are written as without it.  With a static camera and one frame number per call the bounce noise averages out as 1/n;
     * the caller resets the history when the camera moves -- or when vxrt_edit_voxels changes the world.  vxrt_render
     * only (a multi-view launch has no per-view history). */
    float *d_accum;
    int32_t accum_reset;
    int32_t reserved_;
} vxrt_render_flags;

void vxrt_render_flags_default(vxrt_render_flags *flags);
/* d_fb: device BGRA8 framebuffer (bytes b,g,r,a = SDLRenderer.h:8-11 PixelData), W*H*4 bytes
 * (or the compact size, see vxrt_compact_rows).  Asynchronous on the stream. */
int vxrt_render(vxrt_ctx *ctx, uint32_t width, uint32_t height, void *d_fb, const float origin[3],
                const float fwd[3], const float up[3], const float right[3], const vxrt_render_flags *flags);
/* Several views of the resident world in ONE launch (this build's addition; the reference renders one view per
 * RenderScreen call).  Why: a frame ends with a stretch where only the longest ray chains are still running and most
 * of the GPU idles -- at 1080p about a quarter of the launch.  With n views in one launch the persistent kernel's
 * queue runs on into the next view's tiles, so only the last view pays that stretch (measured: 1.37x the rays/s of
 * one-view launches at 1080p).  Every view is exactly the frame vxrt_render would produce for the same camera,
 * frame number and flags.  `flags` applies to all views; its frame_number, d_color_aov, d_hit_aov and d_tile_order
 * are ignored (per-view members below).  1 <= n_views <= 16.  Launches issued on different streams may also be in
 * flight together: up to 64 launches (16 of them multi-view) per context share no state; the call that would exceed that
 * waits on the host for the oldest launch to finish before it reuses its queue head / view slot.  Host calls on a context
 * stay serialised.
 *
 * STREAM CAPTURE (hipStreamBeginCapture on `stream`; tests/test_gpu_capture.py captures in the strictest, global mode and
 * holds the sentences below to the references of the eager paths).
 *   May be captured: vxrt_render, vxrt_render_views and vxrt_trace_batch without stats; vxrt_deinterleave_strips and
 *     vxrt_deinterleave_views; and the purely stream-ordered queries vxrt_read_region, vxrt_move_boxes, vxrt_overlap_boxes,
 *     vxrt_distance_field, vxrt_light_field, vxrt_apply_rule (tests/test_gpu_rule.py), vxrt_loose_step (tests/test_gpu_loose.py), vxrt_extract_surface,
 *     vxrt_downsample_region and vxrt_find_islands; and the
 *     frame denoiser's vxrt_frame_guides and vxrt_denoise_frame, the temporal filter's vxrt_reproject_frame and
 *     vxrt_light_frame (tests/test_gpu_light_frame.py); and the voxel materials' vxrt_material_field and vxrt_material_frame
 *     (tests/test_gpu_material.py; vxrt_material_field_host synchronises and is outside, like every _host call).  Under
 *     capture they allocate nothing, wait for nothing and read no host memory after they return: a captured multi-view
 *     launch stores its views from kernel arguments, which the graph owns.  Every replay gives what the eager call gives.
 *   Refused under capture, with VXRT_ERR_INVALID and a message that names capture: a render launch with frame_number < 0, in
 *     the flags of vxrt_render or in any view of vxrt_render_views (the graph would bake the context counter's value of the
 *     moment: pass explicit frame numbers); vxrt_trace_batch with stats_or_null != NULL and vxrt_nav_field (both synchronise
 *     with the host); and vxrt_render_views on a context that has never issued a multi-view launch -- the view slots are
 *     allocated by the first one, so issue one multi-view launch before capturing (the warm-up rule).  A refusal comes before
 *     anything is enqueued and moves neither the frame counter nor the rings: the capture stays valid and goes on.
 *   collect_stats is allowed: the counters grow once per replay, and vxrt_frame_stats_get after the replays reads them.
 *   What a replay sees.  A graph bakes the ADDRESSES of the world tables, not their contents.  vxrt_edit_voxels and
 *     vxrt_edit_stamps that do not grow the pool change the tables in place (the cell table and the coarse bits never move;
 *     only pool growth moves the pool), so later replays see the edited world: reserve with vxrt_edit_reserve before
 *     capturing and check vxrt_edit_stats.pool_capacity.  After pool growth, vxrt_upload_world, vxrt_build_world_procedural,
 *     vxrt_load_world or any vxrt_stream_* call the old tables are freed: every graph captured before must be captured again.
 *     The environment, the FOV and the ortho window are baked as they were at capture; later vxrt_set_* calls reach only
 *     later launches.
 *   Keeping within the limits.  Inside a capture nothing can be waited for or recorded, so the in-flight limits above are
 *     the caller's: a graph bakes the queue head (and, multi-view, the view slot) its launch took from the rings, resets and
 *     fills them with nodes of its own at every replay, and holds them for the duration of the replay.  Its replays must be
 *     ordered -- on the same stream, or by events -- with each other and with the context's other launches; then any number
 *     of eager launches may come between capture and replay.
 *   Outside the contract: every other call that takes a stream (vxrt_place_pieces, vxrt_voxelize_mesh, vxrt_nav_paths) and
 *     every call that takes none. */
typedef struct vxrt_view {
    void *d_fb;             /* W*H*4 bytes BGRA8 (or the compact size) */
    float origin[3], fwd[3], up[3], right[3];
    int64_t frame_number;   /* as vxrt_render_flags.frame_number */
    float *d_color_aov;     /* optional, as in vxrt_render_flags */
    int64_t *d_hit_aov;
} vxrt_view;
int vxrt_render_views(vxrt_ctx *ctx, uint32_t width, uint32_t height, uint32_t n_views, const vxrt_view *views,
                      const vxrt_render_flags *flags);
/* the kernel (7 or 1) a vxrt_render (nviews = 0) or vxrt_render_views launch of this shape would run under the
 * context's current variant; -1 on bad arguments.  For tools that label measurements by kernel (bench.py). */
int vxrt_kernel_for_launch(const vxrt_ctx *ctx, uint32_t width, uint32_t height, const vxrt_render_flags *flags, uint32_t nviews);
/* 1 when a vxrt_render (nviews = 0) or vxrt_render_views launch of this shape would run the persistent kernel's instantiation
 * for plain shaded frames -- shaded mode, perspective camera, no checkerboard, no strips, no accumulation history, no
 * hit-index AOV, on an ordinary grid with brick edge 32 -- in which those launch flags are compile-time constants; 0 when it runs the general instantiation (or kernel 1, or no world is resident); -1 on bad arguments.  Host
 * only: nothing is launched.  For a multi-view launch a non-NULL flags->d_hit_aov stands for "some view has a hit-index
 * AOV" (only here: vxrt_render_views itself reads the views' own pointers).  The frames are the same bit for bit either way. */
int vxrt_render_specialisation(const vxrt_ctx *ctx, uint32_t width, uint32_t height, const vxrt_render_flags *flags, uint32_t nviews);
/* number of frame rows owned by a shard, = rows of its compact buffer */
uint32_t vxrt_compact_rows(uint32_t height, int32_t strip_rows, int32_t strip_count, int32_t strip_index);
/* counters accumulated by the launches on this context since the previous read, whatever their streams; synchronises
 * the device (every stream).  The device-side counters only grow: "since the previous read" is a host-side snapshot, so a
 * read never clears memory that a running kernel adds to. */
int vxrt_frame_stats_get(vxrt_ctx *ctx, vxrt_frame_stats *out);
/* Loop diagnostics of the persistent render kernel's counting launches that vxrt_frame_stats has no field for, as the LAST
 * vxrt_frame_stats_get on this context read them (their deltas over the same interval; zeros before the first read).  Host
 * only: nothing is synchronised or copied.  Writes min(capacity, n) words to `out` and returns n, the number of counters:
 *   [0] rounds in which both the end-of-walk and the ray-finished phase ran
 *   [1] ... and in which the first restarted a coarse walk and the second launched a ray
 *   [2] bounce samples launched from the end-of-walk phase (a shadowed pixel's sample 0, whose shadow ray never parked)
 * A negative return is an error code. */
int vxrt_loop_counters_get(vxrt_ctx *ctx, uint64_t *out, int32_t capacity);
/* scatter `strip_count` compact shard buffers (laid out back to back, shard-major, each padded to
 * `shard_stride_bytes`) into a full W*H BGRA8 frame on the device; used by the root after the gather. */
int vxrt_deinterleave_strips(vxrt_ctx *ctx, uint32_t width, uint32_t height, int32_t strip_rows,
                             int32_t strip_count, const void *d_shards, uint64_t shard_stride_bytes,
                             void *d_fb, void *stream);
/* the same for the `n_views` views of one multi-view step in ONE launch: view j's packed rows start
 * `j * view_stride_bytes` into every shard's contribution, its frame `j * fb_stride_bytes` into d_fb */
int vxrt_deinterleave_views(vxrt_ctx *ctx, uint32_t width, uint32_t height, int32_t strip_rows, int32_t strip_count,
                            const void *d_shards, uint64_t shard_stride_bytes, uint64_t view_stride_bytes,
                            uint32_t n_views, void *d_fb, uint64_t fb_stride_bytes, void *stream);

/* ---- frame denoiser -- an EXTENSION (the reference's to-do item "Proper indirect lighting (denoise, temporal accumulation,
 * ...)", README.md:19; its screenshots are captioned "no denoise"): an edge-avoiding a-trous filter over the colour AOV of a
 * frame, guided by the voxel face every pixel shows.  Every surface of this renderer is an axis-aligned voxel face, so "the
 * same surface" is an exact integer predicate and the filter is specified bit for bit.  A post-process of two calls over
 * buffers the renderer already writes (vxrt_render_flags.d_color_aov and d_hit_aov); the render launches know nothing of it.
 *   Frames.  Whole frames only: 1 <= W, H <= 65535 and W * H <= 2^26, pixel (x, y) at index x + W * y.  Strips, compact
 *     shards and checkerboard frames are outside the contract (their AOVs hold some of the frame's pixels only).
 *   Guide keys (vxrt_frame_guides).  d_keys[i] is 0 for a miss, else 1<<31 | axis<<26 | toward<<25 | plane with axis 0 .. 2 and
 *     plane < 2^25.  The world sits at the origin with unit voxels; X, Y, Z are its voxel extents (at most 2^24 each).  A hit
 *     index h = x + X * (y + Y * z) in 0 .. X*Y*Z - 1 names the voxel v; -1 and every index outside that range give key 0.
 *     (o, d) is the pixel's primary ray exactly as vxrt_render forms it for the same W, H, camera vectors and `ortho` flag,
 *     under the context's FOV and ortho window at the time of the call.  For each axis k with d[k] != 0: p[k] = d[k] > 0 ?
 *     v[k] : v[k] + 1 and t[k] = (p[k] - o[k]) / d[k], one binary32 subtraction and one IEEE division; an axis with d[k] == 0
 *     has t[k] = -inf (and p[k] = v[k] + 1).  axis = the first k with the largest t[k], toward = d[axis] > 0, plane = p[axis].
 *     This is the face of the voxel's box that the ray enters, defined by this rule alone and not by the tracer's normal.
 *     The call reads the hit AOV and the world's extents, no world table.
 *   Filter (vxrt_denoise_frame).  h = (3/8, 1/4, 1/16) for |offset| = 0, 1, 2.  Iteration i = 0 .. iterations - 1 has step
 *     s = 2^i and maps colour c_i to c_{i+1}, c_0 = d_color_in.  A pixel p with key 0 is copied.  Otherwise, with sw = 0 and
 *     sc = (0, 0, 0), for dy = -2 .. 2 (outer loop) and dx = -2 .. 2 (inner loop) let q = p + s * (dx, dy); q is skipped when
 *     it lies outside the frame or key(q) != key(p); else
 *         w = h[|dx|] * h[|dy|]
 *         if color_scale > 0:  e = c_i(q) - c_i(p) per channel;  d2 = (e.r*e.r + e.g*e.g) + e.b*e.b;
 *                              t = 1 - d2 * color_scale;  w = w * (t > 0 ? t : 0)
 *         sw += w;  sc.ch += w * c_i(q).ch for each channel
 *     and c_{i+1}(p) = sc / sw, three IEEE divisions (the centre tap keeps sw > 0 for finite colours and color_scale).  All
 *     operations are binary32, in this order, without contraction.  The last iteration is stored to d_color_out and, when
 *     d_fb_or_null is given, as a BGRA8 pixel by the rule of the render launches (clamp to 0 .. 1, * 255, truncate; bytes
 *     b, g, r, 255).  d_color_in may be the colour AOV of an accumulated frame (d_accum): the filter then works on the mean.
 *     d_color_out may be d_color_in or overlap it in part.  d_work, d_keys and the outputs must not overlap otherwise.
 *   Workspace.  d_work holds vxrt_denoise_workspace_bytes(W, H) = 2 * W * H * 16 bytes (two buffers of one 16-byte record
 *     {r, g, b, key} per pixel; 0 outside the limits on W and H), 16-byte aligned.  The caller owns it.
 *   Call rules.  Both calls are asynchronous on `stream`, allocate nothing, wait for nothing and read no host memory after
 *     they return; both may be captured (STREAM CAPTURE above).  Refusals, each VXRT_ERR_INVALID before anything is enqueued
 *     or written, checked in this order: a NULL ctx; no world resident (vxrt_frame_guides only); W or H outside the limits;
 *     params NULL or its struct_size; iterations outside 1 .. 6; a color_scale that is negative or NaN; a NULL origin, fwd,
 *     up, right, d_hit_aov or d_keys (guides), a NULL d_color_in, d_keys, d_work or d_color_out (filter); a world axis longer
 *     than 2^24 voxels (guides).
 *   The cost is one launch for the keys and one per iteration: an iteration reads 25 records per filtered pixel, lanes
 *     along x, and writes one; the first reads the float3 colours and the keys instead, the last writes float3 and BGRA8. */
typedef struct vxrt_denoise_params {
    uint32_t struct_size;
    int32_t iterations;   /* 1 .. 6 */
    float color_scale;    /* k >= 0; 0 = no colour stop */
    int32_t reserved_;
} vxrt_denoise_params;
int vxrt_frame_guides(vxrt_ctx *ctx, uint32_t W, uint32_t H, const float origin[3], const float fwd[3], const float up[3],
                      const float right[3], int32_t ortho, const int64_t *d_hit_aov, uint32_t *d_keys, void *stream);
uint64_t vxrt_denoise_workspace_bytes(uint32_t W, uint32_t H); /* 2 * W * H * 16; 0 outside the contract */
int vxrt_denoise_frame(vxrt_ctx *ctx, uint32_t W, uint32_t H, const float *d_color_in /* W*H*3 */, const uint32_t *d_keys,
                       const vxrt_denoise_params *params, void *d_work, float *d_color_out /* W*H*3, may alias d_color_in */,
                       void *d_fb_or_null /* BGRA8 */, void *stream);

/* ---- temporal filter -- an EXTENSION (the same to-do item of the reference, "... temporal accumulation"): the frame history
 * reprojected across camera moves.  vxrt_render_flags.d_accum averages the stochastic bounce term over frames but needs a
 * static camera; this call carries a running mean per pixel from the previous frame to the current one through the surface
 * point every pixel shows.  Every surface is an axis-aligned voxel face and vxrt_frame_guides names it per pixel, so the
 * hit point is "primary ray meets plane", "the previous frame showed the same surface there" is key equality, and the filter
 * is specified bit for bit: no depth or normal heuristics, no tolerances.  A post-process over buffers the renderer and
 * vxrt_frame_guides already write; the render launches know nothing of it and d_accum stays as it is.  A frame pipeline
 * reads: render with AOVs, guide keys, reproject, a-trous over the accumulated mean (d_color_out is a d_color_in of
 * vxrt_denoise_frame).
 *   Frames.  Whole frames with the denoiser's limits: 1 <= W, H <= 65535 and W * H <= 2^26, pixel (x, y) at index x + W * y.
 *     Strips, compact shards and checkerboard frames are outside the contract.
 *   Inputs.  d_color_in (W*H*3) and d_keys (W*H) are the colour AOV and the guide keys of the current frame; d_keys_prev and
 *     d_hist_in are the keys and the d_hist_out of the previous call.  If either of the two is NULL there is no history (the
 *     first frame, or the caller's reset): no tap is accepted.  The caller ping-pongs two history and two key buffers, and
 *     resets after vxrt_edit_voxels / vxrt_edit_stamps (shadows and bounces change far from an edit's box) and after a change
 *     of the FOV or the ortho window.  A record is {r, g, b, n}: the mean and the number of frames in it, 0 on a miss pixel.
 *   Camera constants.  Both cameras use the context's FOV and ortho window at the time of the call and params->ortho: kx, ky,
 *     ortho_x, ortho_y and ratio below are the per-launch constants of the render launches (kx = tan(fov / 2) * (W / H),
 *     ky = tan(fov / 2), ratio = W / H, ortho_x and ortho_y the ortho window).
 *   All arithmetic is binary32, in the order written, without contraction.  For pixel p = (x, y) with colour c and key k:
 *     1. Miss.  k == 0: the record is {c, 0}; the pixel counts nowhere.
 *     2. Hit point.  `hit` is counted.  a = the key's axis, pl = (float)plane.  (o, d) is the pixel's primary ray under `cur`
 *        exactly as vxrt_render forms it (the ray of vxrt_frame_guides).  t = (pl - o[a]) / d[a]; if d[a] == 0 or t is not
 *        finite the pixel is offscreen.  P[j] = o[j] + t * d[j] for j != a (one multiply, one add), P[a] = pl.
 *     3. Into the previous camera.  r = P - prev.origin; dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z.
 *        Perspective: z = dot(r, prev.fwd); the pixel is offscreen unless z > 0; su = dot(r, prev.right) / (z * kx),
 *        sv = dot(r, prev.up) / (z * ky).  Ortho: su = dot(r, prev.right) / (ortho_x * ratio), sv = dot(r, prev.up) / ortho_y.
 *        fx = ((su + 1) * 0.5f) * (float)W and fy likewise with H (pixel x looks through u = x / W, so an integer fx is a
 *        pixel exactly).  The pixel is offscreen unless fx >= -1 && fx <= W && fy >= -1 && fy <= H (a NaN fails).
 *     4. Taps.  x0 = floor(fx), wx = fx - x0; y0 and wy likewise.  The four taps, in this order: (x0, y0), (x0+1, y0),
 *        (x0, y0+1), (x0+1, y0+1), with weights (1-wx)*(1-wy), wx*(1-wy), (1-wx)*wy, wx*wy.  A tap q is accepted when it lies
 *        in the frame, its weight is > 0, keys_prev(q) == k and hist_in(q).n >= 1.  With sw = 0, sc = (0, 0, 0) and
 *        nmin = +inf, an accepted tap does sw += w, sc.ch += w * hist_in(q).ch per channel and nmin = min(nmin, hist_in(q).n).
 *        A tap that is not accepted leaves the sums untouched -- a select, not an addition of zero: a NaN behind a foreign
 *        key stays out, as in the denoiser.
 *     5. Blend.  If no tap lies in the frame the pixel is offscreen; else, if none is accepted, it is rejected (a
 *        disocclusion).  Both give the record {c, 1}.  Otherwise the pixel is reused: m = sc / sw per channel,
 *        n' = min(nmin + 1, (float)max_history), out = m + (c - m) / n' (one subtract, one divide, one add); record {out, n'}.
 *     6. Outputs.  d_hist_out takes the record, d_color_out (if given) its rgb, d_fb (if given) the BGRA8 pixel by the rule
 *        of the render launches (clamp to 0 .. 1, * 255, truncate; bytes b, g, r, 255).  d_summary (if given) is zeroed on
 *        the stream by the call and then takes the four counts: hit = reused + offscreen + rejected.
 *   Why key equality is enough.  P lies on plane k by construction.  If the previous pixel q showed plane k from the same
 *     side, then q's ray met that plane within about a pixel's footprint of P -- the same surface point, up to the footprint
 *     every bilinear tap has.  Two faces of one plane and side that are apart in the world are apart in the frame as well.
 *   Aliasing.  d_color_out may be d_color_in.  d_hist_out must not overlap d_hist_in.  Nothing else may overlap.
 *   Call rules.  Asynchronous on `stream`; allocates nothing, waits for nothing and reads no host memory after it returns;
 *     may be captured (STREAM CAPTURE above).  No world is needed: the keys carry the geometry.  Refusals, each
 *     VXRT_ERR_INVALID before anything is enqueued or written, checked in this order: a NULL ctx; W or H outside the limits;
 *     params NULL or its struct_size; max_history outside 1 .. 65535 or a nonzero reserved_; a non-finite component in either
 *     pose; a NULL d_color_in, d_keys or d_hist_out.
 *   The cost is one launch (and one 16-byte memset with a summary): per pixel 16 bytes read of its own, four 16-byte records
 *     and four keys of the previous frame, which neighbouring lanes largely share, and 32 bytes written. */
typedef struct vxrt_history { float r, g, b, n; } vxrt_history; /* 16 bytes, 16-byte aligned; n = frames in the mean */
typedef struct vxrt_camera_pose { float origin[3], fwd[3], up[3], right[3]; } vxrt_camera_pose;
typedef struct vxrt_reproject_params {
    uint32_t struct_size;
    int32_t ortho;
    int32_t max_history;  /* 1 .. 65535 */
    int32_t reserved_;    /* 0 */
    vxrt_camera_pose cur, prev;
} vxrt_reproject_params;
typedef struct vxrt_reproject_summary { uint32_t hit, reused, offscreen, rejected; } vxrt_reproject_summary;
int vxrt_reproject_frame(vxrt_ctx *ctx, uint32_t W, uint32_t H, const float *d_color_in, const uint32_t *d_keys,
                         const vxrt_history *d_hist_in_or_null, const uint32_t *d_keys_prev_or_null,
                         const vxrt_reproject_params *params, vxrt_history *d_hist_out,
                         float *d_color_out_or_null, void *d_fb_or_null,
                         vxrt_reproject_summary *d_summary_or_null, void *stream);

/* ---- light on frames -- an EXTENSION (the reference's to-do items "Proper indirect lighting" and "Post process stack",
 * README.md:14-24, in the voxel-engine form: per-vertex "smooth lighting" and the three-neighbour corner occlusion on every
 * voxel face).  vxrt_light_field computes sky and emitter light for a box of the world; this call turns those levels into
 * pixels.  Every surface is an axis-aligned voxel face; the guide key and the hit index name the face a pixel shows, so the
 * stage is specified bit for bit, like the denoiser and the temporal filter.  A post-process over buffers the renderer,
 * vxrt_frame_guides and vxrt_light_field already write; the render launches know nothing of it.  In a frame pipeline it
 * is the last stage: render with AOVs, guide keys, reproject, a-trous, light.
 *   All float arithmetic is binary32, in the order written, without contraction.
 *   Frames.  Whole frames with the denoiser's limits: 1 <= W, H <= 65535 and W * H <= 2^26, pixel (x, y) at index x + W * y.
 *     d_keys are the keys vxrt_frame_guides gives for params->cam, params->ortho and the same d_hit_aov (a key whose axis
 *     field is above 2 is read as axis 2).  X, Y, Z are the world's voxel extents, at most 2^24 each.
 *   Miss.  A pixel is a miss when its key is 0 or its hit index lies outside 0 .. X*Y*Z - 1.  Its colour is copied, its terms
 *     are (0, 0, 0) and it counts nowhere.
 *   Face.  v is the voxel of the hit index h = v.x + X * (v.y + Y * v.z), a the key's axis, (b, c) the other two axes in
 *     ascending order, e_k the unit vector of axis k.  The front cell is f = v - e_a when the key's toward bit is set, else
 *     v + e_a.
 *   Position on the face.  (o, d) is the pixel's primary ray under params->cam exactly as vxrt_render forms it (the ray of
 *     vxrt_frame_guides).  t = ((float)plane - o[a]) / d[a]; u = (o[b] + t * d[b]) - (float)v[b] (one multiply, one add, one
 *     subtract) and w likewise on axis c.  Each is then clamped by x < 0 ? 0 : x > 1 ? 1 : x (an infinity becomes 0 or 1, a
 *     NaN stays).  If d[a] == 0, or t, u or w is not finite, then u = w = 0.5f: the centre of the face.
 *   Cells.  cell(i, j) = f + i * e_b + j * e_c for i, j in {-1, 0, 1}: the nine cells in front of the face.  solid(q) is the
 *     world's voxel; a voxel outside the world is empty, as for every query.  lev(q) is 0 for a solid q; otherwise the byte
 *     of d_levels at q - box_origin in region order (x fastest, then y, then z: the d_levels of vxrt_light_field for the
 *     box B = [box_origin, box_origin + box_dims)) when q lies in B and d_levels is given; otherwise outside_level.  The
 *     sky nibble of a byte is its high one, the block nibble its low one.
 *   Corner (i, j) in {0, 1}^2, with si = 2i - 1 and sj = 2j - 1: s1 = solid(cell(si, 0)), s2 = solid(cell(0, sj)),
 *     s3 = solid(cell(si, sj)).  The members are cell(0, 0) always, cell(si, 0) unless s1, cell(0, sj) unless s2, and
 *     cell(si, sj) unless s3 || (s1 && s2): light does not leak through a closed corner.  cnt = the number of members,
 *     1 .. 4.  LS = (float)(sum of the members' sky nibbles) / (float)cnt, LB likewise with the block nibbles.
 *     open = (s1 && s2) ? 0 : 3 - (s1 + s2 + s3) and A = ao_curve[open].  Without VXRT_LF_SMOOTH every corner has LS and LB
 *     equal to the nibbles of lev(cell(0, 0)) as floats; without VXRT_LF_OCCLUSION every corner has A = 1.0f.
 *   Interpolation.  For each of LS, LB and A, with i along b and j along c, each step one subtract, one multiply, one add:
 *     q0 = q00 + u * (q10 - q00);  q1 = q01 + u * (q11 - q01);  q = q0 + w * (q1 - q0).
 *   Colour.  S = LS / 15.0f and Bk = LB / 15.0f; ks = sky_floor + (1.0f - sky_floor) * S; per channel
 *     out = (c * ks + block_color[ch] * Bk) * A.
 *   Stores.  d_color_out takes out (the copied colour on a miss), d_fb (if given) the BGRA8 pixel of what d_color_out takes
 *     by the rule of the render launches (clamp to 0 .. 1, * 255, truncate; bytes b, g, r, 255), d_terms (if given) the
 *     three floats (S, Bk, A) per pixel.  d_summary (if given) is zeroed on the stream by the call and then counts: hit (hit
 *     pixels); in_box (hit pixels with f in B and d_levels given); occluded (hit pixels of which some corner has open < 3,
 *     counted whether or not VXRT_LF_OCCLUSION is set); dark (hit pixels with S == 0 and Bk == 0).
 *   Aliasing.  d_color_out may be d_color_in.  Nothing else may overlap.
 *   Call rules.  The call needs a resident world that is not streamed.  It is asynchronous on `stream`, allocates nothing,
 *     waits for nothing, reads no host memory after it returns and may be captured (STREAM CAPTURE above).  It never loads
 *     outside the world tables and never outside the box_dims[0] * box_dims[1] * box_dims[2] bytes of d_levels.  Refusals,
 *     each before anything is enqueued or written, checked in this order: a NULL ctx; W or H outside the limits; params NULL
 *     or its struct_size; flags with a bit other than the two, outside_level > 0xFF or a nonzero reserved_; sky_floor outside
 *     0 .. 1 or NaN; a block_color or ao_curve entry that is negative or not finite; a non-finite component of the pose;
 *     box dims outside vxrt_light_field's limits on dims (1 <= box_dims[k], their product <= 2^28) or
 *     box_origin[k] + box_dims[k] > 2^31 - 1; a NULL d_color_in, d_keys, d_hit_aov or d_color_out -- each VXRT_ERR_INVALID;
 *     then no world: VXRT_ERR_NO_WORLD; then a streamed world, then a world axis longer than 2^24 voxels: VXRT_ERR_INVALID.
 *   The cost is one launch (and one 16-byte memset with a summary): per hit pixel nine cell records, nine brick words and
 *     nine level bytes, which neighbouring lanes largely share, 24 bytes read of its own and 12 .. 28 bytes written. */
#define VXRT_LF_SMOOTH 1u
#define VXRT_LF_OCCLUSION 2u
typedef struct vxrt_light_frame_params {
    uint32_t struct_size;
    int32_t ortho;
    uint32_t flags;          /* VXRT_LF_SMOOTH | VXRT_LF_OCCLUSION; other bits are invalid */
    uint32_t outside_level;  /* (sky << 4) | block of an empty cell outside the light box; <= 0xFF */
    float sky_floor;         /* 0 .. 1: what stays of a colour where no sky light reaches */
    float block_color[3];    /* finite, >= 0: the colour emitter light adds at level 15 */
    float ao_curve[4];       /* finite, >= 0: the factor of a corner with 0, 1, 2, 3 open neighbours */
    vxrt_camera_pose cam;    /* the pose the frame was rendered with */
    int32_t box_origin[3], box_dims[3]; /* the box B of the vxrt_light_field call */
    int32_t reserved_;       /* 0 */
} vxrt_light_frame_params;
typedef struct vxrt_light_frame_summary { uint32_t hit, in_box, occluded, dark; } vxrt_light_frame_summary;
int vxrt_light_frame(vxrt_ctx *ctx, uint32_t W, uint32_t H, const float *d_color_in, const uint32_t *d_keys,
                     const int64_t *d_hit_aov, const uint8_t *d_levels_or_null, const vxrt_light_frame_params *params,
                     float *d_color_out, void *d_fb_or_null, float *d_terms_or_null /* W*H*3: S, Bk, A */,
                     vxrt_light_frame_summary *d_summary_or_null, void *stream);

/* ---- voxel materials -- an EXTENSION (the reference's to-do item "Texture mapping and materials", README.md:14-24; its
 * calculateColor has no albedo: every surface is white).  A world is one bit per voxel, so the material of a voxel is a pure
 * function of the world's geometry -- terrain strata by altitude band: a top material, a layer under it, a deep one -- with an
 * optional caller-owned byte box of paint on top.  vxrt_material_field gives the material bytes of a box; vxrt_material_frame
 * multiplies the colours of a frame with tint and texture of the material each hit pixel shows.  Both use the same per-voxel
 * function; the render launches know nothing of either.
 *   The material of a voxel.  Material ids are 1 .. 255; 0 is "empty" in a field and "not painted" in a paint box.  +y is
 *     up; a voxel outside the world is empty.  run(v) is the number of consecutive solid voxels directly above v, at
 *     (v.x, v.y + j, v.z) for j = 1, 2, ...  band(v) is the last i < n_bands with bands[i].y_from <= v.y.  With
 *     b = bands[band(v)]: rule(v) = b.top when run(v) == 0, b.under when 1 <= run(v) <= b.under_depth, else b.deep.  No
 *     implementation looks more than under_depth + 1 <= 16 voxels up.
 *   Rules.  n_bands is 1 .. 8; bands[0].y_from == INT32_MIN and y_from ascends strictly over the bands in use; top, under
 *     and deep are 1 .. 255, under_depth is 0 .. 15 (bands at and behind n_bands are not looked at); reserved_ is 0.
 *   Paint.  d_paint, optional, holds one byte per voxel of the box P = [paint_origin, paint_origin + paint_dims) in region
 *     order (x fastest, then y, then z).  material(v) is that byte when d_paint is given, v lies in P and the byte is not 0;
 *     otherwise rule(v).  paint_dims and paint_origin are checked only when d_paint is given, with the limits of
 *     vxrt_light_frame's box: 1 <= paint_dims[k], their product <= 2^28, paint_origin[k] + paint_dims[k] <= 2^31 - 1.
 *   Field (vxrt_material_field).  d_materials takes one byte per voxel of B = [origin, origin + dims) in region order: 0
 *     for an empty voxel, material(v) otherwise.  d_summary is zeroed on the stream by the call and then counts: solid;
 *     painted (solid voxels whose material came from paint); top (solid voxels with run == 0); hist[m] (voxels by output
 *     byte: hist[0] the empty voxels of B).  Limits: 1 <= dims[k], their product <= 2^28, origin[k] >= -2^31 and
 *     origin[k] + dims[k] + 16 <= 2^31 - 1.  No workspace.  d_paint, d_materials and d_summary must not overlap.
 *     vxrt_material_field_host takes host buffers (paint in; materials and summary out), allocates its own device memory
 *     and synchronises.
 *   Field call rules (as vxrt_light_field).  Asynchronous on `stream`; allocates nothing, never synchronises, reads no host
 *     memory after it returns; may be captured (STREAM CAPTURE above).  It never loads outside the world tables, outside the
 *     paint_dims[0] * paint_dims[1] * paint_dims[2] bytes of d_paint or behind d_materials, and writes exactly dims[0] *
 *     dims[1] * dims[2] bytes and the summary.  Two calls give the same bytes.  Refusals, each before anything is enqueued
 *     or written, in this order: a NULL ctx, origin, dims, rules, d_materials or d_summary; rules->struct_size; n_bands; a
 *     band (y_from, a material 0, under_depth > 15); reserved_; the paint box when d_paint is given; dims; origin -- each
 *     VXRT_ERR_INVALID; then no world: VXRT_ERR_NO_WORLD; then a streamed world: VXRT_ERR_INVALID.
 *   Frame (vxrt_material_frame).  Frames, keys, the miss rule, the voxel v, the axis a with (b, c), the primary ray, t, the
 *     position (u, w) on the face with its clamps and its centre fallback, and the BGRA8 store are exactly those of
 *     vxrt_light_frame.  All float arithmetic is binary32, in the order written, without contraction.
 *     Face class: a == 1 with the key's toward bit clear is a top face, a == 1 with it set a bottom face, every other face a
 *     side face.  With m = material(v), tile = d_palette[m].tile_top, tile_bottom or tile_side by that class.
 *     Texel: T = 1 << tile_shift; iu = min((int)(u * (float)T), T - 1) and iw likewise from w.  Column s and row r (image rows
 *     top-down): a == 1: s = iu, r = iw; a == 0 (b = y, c = z): s = iw, r = T - 1 - iu; a == 2 (b = x, c = y): s = iu,
 *     r = T - 1 - iw.  The atlas is RGBA8 packed in a uint32, r in the low byte, tile-major and row-major inside a tile:
 *     texel = d_atlas[(tile * T + r) * T + s].  If d_atlas is NULL or tile >= n_tiles (0xFFFF: "none") the texel colour is
 *     (1, 1, 1) and nothing is loaded -- the palette's contents cannot be checked on the host; this rule keeps every load
 *     inside the n_tiles * T * T words of the atlas.  Otherwise tex.ch = (float)byte / 255.0f, an IEEE division.
 *     Colour, per channel: alb = tint[ch] * tex.ch; out = c * alb.  The colour AOV is what the pixel store gets, after the
 *     renderer's tonemap; multiplying there is deliberate, as in vxrt_light_frame.  In a frame pipeline the stage runs after
 *     the a-trous filter (which then works on demodulated lighting) and before vxrt_light_frame.
 *     A miss copies its colour, writes 0 to the material AOV and counts nowhere.
 *     Outputs: d_color_out (may be d_color_in; nothing else may overlap), d_fb (if given) the BGRA8 pixel of it,
 *     d_material_aov (if given) m per pixel, d_summary (if given; zeroed on the stream by the call): hit; painted (hit pixels
 *     whose material came from paint); top (hit pixels with run(v) == 0); textured (hit pixels that loaded a texel).
 *   Frame call rules (as vxrt_light_frame).  Needs a resident world that is not streamed; asynchronous on `stream`, allocates
 *     nothing, waits for nothing, reads rules and params before it returns and no host memory after; may be captured.
 *     Refusals, each before anything is enqueued or written, in this order: a NULL ctx; W or H outside the limits; params
 *     NULL or its struct_size; n_tiles > 4096, tile_shift > 6 or a nonzero reserved_; the rules (as above: NULL or
 *     struct_size, n_bands, a band, reserved_); a non-finite component of the pose; the paint box when d_paint is given; a
 *     NULL d_color_in, d_keys, d_hit_aov, d_palette or d_color_out -- each VXRT_ERR_INVALID; then no world:
 *     VXRT_ERR_NO_WORLD; then a streamed world, then a world axis longer than 2^24 voxels: VXRT_ERR_INVALID.
 *   The cost.  Field: one launch and one memset; a lane owns four x-consecutive voxels and marches down y, one row word of
 *     the world per 32 voxels and row, 16 rows of warm-up per y segment.  Frame: one launch (and a 16-byte memset with a
 *     summary); per hit pixel up to under_depth + 2 solidity lookups, one palette entry and one texel. */
#define VXRT_MATERIAL_MAX_BANDS 8
#define VXRT_MATERIAL_NO_TILE 0xFFFFu
typedef struct vxrt_material_band {
    int32_t y_from;       /* the band holds the voxels with y >= y_from, below the next band's y_from */
    uint8_t top, under, deep;  /* material ids, 1 .. 255 */
    uint8_t under_depth;  /* 0 .. 15: how many voxels of `under` lie below a top voxel */
} vxrt_material_band;
typedef struct vxrt_material_rules {
    uint32_t struct_size;
    uint32_t n_bands;     /* 1 .. 8 */
    vxrt_material_band bands[VXRT_MATERIAL_MAX_BANDS];
    int32_t paint_origin[3], paint_dims[3]; /* the box P of d_paint; looked at only when d_paint is given */
    int32_t reserved_;    /* 0 */
} vxrt_material_rules;
typedef struct vxrt_material_summary { uint32_t solid, painted, top, reserved; uint32_t hist[256]; } vxrt_material_summary;
typedef struct vxrt_material {     /* a palette entry, 20 bytes; entry m belongs to material m */
    float tint[3];
    uint16_t tile_top, tile_side, tile_bottom; /* atlas tiles; >= n_tiles (VXRT_MATERIAL_NO_TILE): no texture */
    uint16_t reserved;
} vxrt_material;
typedef struct vxrt_material_frame_params {
    uint32_t struct_size;
    int32_t ortho;
    uint32_t n_tiles;      /* tiles in d_atlas, <= 4096 */
    uint32_t tile_shift;   /* 0 .. 6: a tile is T x T texels, T = 1 << tile_shift */
    vxrt_camera_pose cam;  /* the pose the frame was rendered with */
    int32_t reserved_;     /* 0 */
} vxrt_material_frame_params;
typedef struct vxrt_material_frame_summary { uint32_t hit, painted, top, textured; } vxrt_material_frame_summary;
int vxrt_material_field(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_material_rules *rules,
                        const uint8_t *d_paint_or_null, uint8_t *d_materials, vxrt_material_summary *d_summary, void *stream);
int vxrt_material_field_host(vxrt_ctx *ctx, const int32_t origin[3], const int32_t dims[3], const vxrt_material_rules *rules,
                             const uint8_t *paint_or_null, uint8_t *materials, vxrt_material_summary *summary);
int vxrt_material_frame(vxrt_ctx *ctx, uint32_t W, uint32_t H, const float *d_color_in, const uint32_t *d_keys,
                        const int64_t *d_hit_aov, const vxrt_material_rules *rules, const uint8_t *d_paint_or_null,
                        const vxrt_material *d_palette /* 256 entries */, const uint32_t *d_atlas_or_null,
                        const vxrt_material_frame_params *params, float *d_color_out, void *d_fb_or_null,
                        uint8_t *d_material_aov_or_null, vxrt_material_frame_summary *d_summary_or_null, void *stream);

/* ---- sky on frames -- an EXTENSION (the reference's to-do item "Sky rendering", README.md:14-24; its setPixelColor stores the
 * primary ray's direction as the colour of a pixel that misses the world, Renderer.cu:254-257, and every stage above copies
 * that colour).  This call gives every miss pixel a sky -- a gradient from horizon to zenith, a ground colour below the
 * horizon, a sun glow and a sun disc, a layer of value-noise clouds on a plane -- and fades every hit pixel towards the sky
 * behind it with the distance of its surface point (aerial perspective).  A post-process over buffers the renderer and
 * vxrt_frame_guides already write; the render launches know nothing of it.  In a frame pipeline it is the last stage:
 * render with AOVs, guide keys, reproject, a-trous, materials, light, sky.  The colour AOV is the colour handed to the pixel
 * store, after the tonemap: the stage works in display space, 0 .. 1.
 *   Frames.  Whole frames with the denoiser's limits: 1 <= W, H <= 65535 and W * H <= 2^26, pixel (x, y) at index x + W * y.
 *     d_keys are the keys vxrt_frame_guides gives for params->cam and params->ortho.  No world is needed: the keys carry the
 *     geometry.  The camera constants are the context's FOV and ortho window at the time of the call and params->ortho.
 *   Arithmetic.  All float arithmetic is binary32, in the order written, without contraction: add, subtract, multiply, IEEE
 *     divide, compare, select, floorf and conversions between int32 and float; the one square root is taken on the host.
 *     dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z;  clamp01(x) = x < 0 ? 0 : x > 1 ? 1 : x (a NaN stays);
 *     mix(a, b, w) = a + (b - a) * w (one subtract, one multiply, one add);  smooth(x) = (x * x) * (3 - 2 * x).
 *   Ray.  (o, d) is the pixel's primary ray under params->cam exactly as vxrt_render forms it (the ray of vxrt_frame_guides);
 *     h = d.y (+y is up).
 *   Sun.  s = sun_dir / n per component with n = sqrtf(dot(sun_dir, sun_dir)), once on the host; sd = dot(d, s).
 *   base(d), the sky without disc and clouds, per channel:
 *     h >= 0:  a = 1 - h; a2 = a * a; a4 = a2 * a2; c = mix(zenith, horizon, a4).  g = sd > 0 ? sd : 0, then g = g * g
 *       glow_log2 times; c = c + sun_color * (glow_strength * g).
 *     otherwise (h < 0, or a NaN):  c = mix(horizon, ground, clamp01((-h) * ground_fade)).  No glow.
 *   Miss pixel (key 0).  c = base(d); what d_color_in holds there is not looked at.  For h >= 0 two further steps:
 *     Disc.  e = smooth(clamp01((sd - cos_outer) / (cos_inner - cos_outer))); c = mix(c, sun_color, e).
 *     Clouds, only with VXRT_SKY_CLOUDS, and only when every condition of this list holds (else the pixel has no cloud):
 *       h > 0 and o.y < cloud_y;  t = (cloud_y - o.y) / h is finite and t <= cloud_max_t;
 *       px = (o.x + t * d.x) * cloud_scale + cloud_offset[0] and pz = (o.z + t * d.z) * cloud_scale + cloud_offset[1] satisfy
 *       -2^30 < px * S < 2^30 and likewise pz, with S = (float)2^(octaves - 1): every cell of every octave converts to int32
 *       exactly.
 *       n = 0; for i = 0 .. octaves - 1 in ascending order: n = n + (float)2^-(i+1) * vnoise(px * (float)2^i, pz * (float)2^i,
 *       seed + i).  dens = clamp01((n - (1 - cloud_cover)) * cloud_sharp); alpha = dens * clamp01(h * cloud_fade);
 *       c = mix(c, cloud_color, alpha).
 *     vnoise(qx, qz, k): fx = floorf(qx), ix = (int32)fx, wx = smooth(qx - fx); fz, iz and wz likewise.  With
 *       v(i, j) = value(ix + i, iz + j, k): x0 = mix(v(0,0), v(1,0), wx); x1 = mix(v(0,1), v(1,1), wx); the result is
 *       mix(x0, x1, wz).
 *     value(i, j, k), all in uint32 wraparound arithmetic: m = (uint32)i * 0x8DA6B343 ^ (uint32)j * 0xD8163841 ^
 *       k * 0xCB1AB31F;  m ^= m >> 16; m *= 0x7FEB352D;  m ^= m >> 15; m *= 0x846CA68B;  m ^= m >> 16;  the value is
 *       (float)(m >> 8) * 2^-24, in 0 .. 1 - 2^-24.
 *   Hit pixel (key != 0): aerial perspective.  a = the key's axis (a field above 2 reads as 2), pl = (float)plane,
 *     t = (pl - o[a]) / d[a].  If d[a] == 0, or t is not finite, or t < 0, the colour is copied.  Otherwise
 *     u = t - fog_start; u = u > 0 ? u : 0; x = u * fog_density; f = x / (1 + x); f = f < fog_max ? f : fog_max (a NaN f, from
 *     an infinite x, becomes fog_max).  If f > 0 the pixel is fogged: out = mix(c_in, base(d), f) per channel -- the fog takes
 *     the colour of the sky behind the surface, sun-side glow included.  Otherwise the colour is copied: fog_density == 0 or
 *     fog_max == 0 copies every hit bit for bit (a mix with f = 0 would turn -0 into +0 and an infinity into a NaN).
 *   Stores.  d_color_out takes out, d_fb (if given) the BGRA8 pixel of it by the rule of the render launches (clamp to
 *     0 .. 1, * 255, truncate; bytes b, g, r, 255).  d_summary (if given) is zeroed on the stream by the call and then counts:
 *     miss and hit (miss + hit = W * H); ground (misses with h < 0); sun (misses with e > 0); cloud (misses with alpha > 0);
 *     fogged (hits with f > 0).
 *   Aliasing.  d_color_out may be d_color_in.  Nothing else may overlap.
 *   Call rules.  Asynchronous on `stream`; allocates nothing, waits for nothing and reads no host memory after it returns;
 *     may be captured (STREAM CAPTURE above).  Refusals, each VXRT_ERR_INVALID before anything is enqueued or written, checked
 *     in this order: a NULL ctx; W or H outside the limits; params NULL or its struct_size; a flag bit other than
 *     VXRT_SKY_CLOUDS or a nonzero reserved_; a component of zenith, horizon, ground, sun_color or cloud_color that is negative
 *     or not finite; glow_log2 above 8, or octaves outside 1 .. 6; one of glow_strength, ground_fade, cloud_scale, cloud_max_t,
 *     cloud_cover, cloud_sharp, cloud_fade, fog_start, fog_density, fog_max that is negative, NaN or infinite, or a cloud_y or
 *     cloud_offset entry that is not finite; fog_max or cloud_cover above 1; cos_inner <= cos_outer, or either outside -1 .. 1
 *     (a NaN fails); a sun_dir whose n is zero or not finite; a non-finite component of the pose; a NULL d_color_in, d_keys or
 *     d_color_out.
 *   The cost is one launch (two with a summary: one wave zeroes it first): per pixel 4 .. 16 bytes read and 12 .. 16 written; a
 *     cloud pixel evaluates four hashes and two smooth weights per octave. */
#define VXRT_SKY_CLOUDS 1u
typedef struct vxrt_sky_params {
    uint32_t struct_size;
    int32_t ortho;
    uint32_t flags;          /* VXRT_SKY_CLOUDS; other bits are invalid */
    uint32_t glow_log2;      /* 0 .. 8: the glow is max(sd, 0) ^ (2 ^ glow_log2) */
    uint32_t octaves;        /* 1 .. 6 */
    uint32_t seed;           /* of the cloud noise */
    float zenith[3], horizon[3], ground[3], sun_color[3], cloud_color[3]; /* finite, >= 0 */
    float sun_dir[3];        /* towards the sun; any length */
    float glow_strength, ground_fade;
    float cos_inner, cos_outer; /* -1 <= cos_outer < cos_inner <= 1: the disc is full inside cos_inner, gone outside cos_outer */
    float cloud_y, cloud_scale, cloud_offset[2], cloud_max_t, cloud_cover /* 0 .. 1 */, cloud_sharp, cloud_fade;
    float fog_start, fog_density, fog_max /* 0 .. 1 */;
    vxrt_camera_pose cam;    /* the pose the frame was rendered with */
    int32_t reserved_;       /* 0 */
} vxrt_sky_params;           /* 208 bytes */
typedef struct vxrt_sky_summary { uint32_t miss, hit, ground, sun, cloud, fogged; } vxrt_sky_summary;
int vxrt_sky_frame(vxrt_ctx *ctx, uint32_t W, uint32_t H, const float *d_color_in, const uint32_t *d_keys,
                   const vxrt_sky_params *params, float *d_color_out, void *d_fb_or_null,
                   vxrt_sky_summary *d_summary_or_null, void *stream);

/* ---- batch query.  Replaces VoxelRaytracer3D::Raytrace + kernel dispatch
 * (VoxelRT/VolumeRaytracer.cu:95-117,574-618).  Results follow the reference
 * convention: miss -> point = +inf; normal (step direction, zero on a miss) and
 * steps always written.  d_hit / d_voxel (optional) are this build's additions:
 * hit flag and global hit voxel index x + X*(y + Y*z), -1 on a miss. */
/* RAY VALIDITY (defined by this build; the reference leaves it undefined): a ray is valid when its origin's components
 * are finite (their absolute sum is a finite binary32) and the squared length of its direction, evaluated in binary32, is
 * positive and finite -- i.e. normalize(direction) is a vector of finite numbers.  NaN or infinite components, the zero
 * direction, and directions so short or long that the squared length leaves the binary32 range make Raytrace's prologue
 * (VolumeRaytracer.cu:359-367) produce NaN, which the reference then casts to int (undefined).  An INVALID ray of a batch
 * is not traced: its result is a miss with 0 steps (point = +inf, normal = 0, d_hit = 0, d_voxel = -1); it is counted as
 * a ray.  vxrt_render / vxrt_render_views return VXRT_ERR_INVALID for a camera with a non-finite component.
 * vxrt_set_environment returns VXRT_ERR_INVALID, and keeps the context's environment, for a light_dir with a non-finite
 * component or whose squared length, evaluated in binary32, is 0 or not finite: its unit vector -- the direction of every
 * shadow ray -- would not be a finite vector.  Any other light_dir, light colour and ambient is accepted. */
int vxrt_trace_batch(vxrt_ctx *ctx, const float *d_origins, const float *d_dirs, uint64_t n, float *d_pos,
                     float *d_normal, int32_t *d_steps, uint8_t *d_hit, int64_t *d_voxel,
                     vxrt_frame_stats *stats_or_null, void *stream);
/* The device function's first argument, `Raytrace(int maxSteps, ...)` (VolumeRaytracer.cu:354): the budget that is tested
 * at the head of the two-level loop only (:386).  The batch kernel of the reference passes MAX_STEPS = 2048 (:105), the
 * secondary rays of calculateColor pass 8 (Renderer.cu:141).  Applies to the following vxrt_trace_batch* calls on this
 * context; default 2048.  1 <= max_steps <= 2048. */
int vxrt_set_batch_max_steps(vxrt_ctx *ctx, int32_t max_steps);
/* host-pointer convenience with the reference's copy-in / copy-out behaviour */
int vxrt_trace_batch_host(vxrt_ctx *ctx, const float *origins, const float *dirs, uint64_t n, float *pos,
                          float *normal, int32_t *steps, uint8_t *hit, int64_t *voxel,
                          vxrt_frame_stats *stats_or_null);

#ifdef __cplusplus
}
#endif
#endif /* VXRT_H */
