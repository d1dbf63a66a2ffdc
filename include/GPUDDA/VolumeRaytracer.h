// GPUDDA/VolumeRaytracer.h -- the reference's VoxelRT/VolumeRaytracer.cuh API surface, re-implemented for
// MI355X as a thin C++ facade over the C ABI in include/vxrt.h (libvxrt.so).  Same namespace, type and member
// names and argument meaning as the reference so VoxelApp-style callers compile against it; nothing here is
// CUDA and no reference source is reused.  float3/uint3 come from <hip/hip_vector_types.h>.
//
// Deliberate differences: device tables are one flat pool instead of one allocation per brick
// (VolumeRaytracer.cu:552-565); Get*() accessors return opaque handles; Raytrace() sizes its result buffers from
// the request instead of the constructor count (VolumeRaytracer.cuh:318-331); voxelIndex is the global voxel
// index of the hit (x + X*(y + Y*z), -1 on a miss or if it does not fit an int) instead of the reference's
// float expression on coarse dimensions (VolumeRaytracer.cu:611-612).
#pragma once

#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>
#include <ostream>
#include <limits>
#include <memory>
#include <tuple>
#include <vector>

struct vxrt_ctx;
struct vxrt_edit_op;     // include/vxrt.h
struct vxrt_edit_stats;
struct vxrt_body;
struct vxrt_island;
struct vxrt_island_summary;
struct vxrt_piece;
struct vxrt_placement;
struct vxrt_placed;
struct vxrt_nav_agent;
struct vxrt_nav_summary;
struct vxrt_distance_summary;
struct vxrt_voxelize_summary;
struct vxrt_quad;
struct vxrt_surface_summary;
struct vxrt_lod_summary;
struct vxrt_light_summary;
struct vxrt_material_rules;
struct vxrt_material_summary;
struct vxrt_rule;
struct vxrt_rule_summary;
struct vxrt_loose;
struct vxrt_loose_summary;

constexpr auto FLT_EPS_DDA = 1e-6;  // VolumeRaytracer.cuh:20 (a double)
constexpr auto FLT_INF = std::numeric_limits<float>::infinity();
constexpr auto FLT_EPS = std::numeric_limits<float>::epsilon();

namespace GPUDDA {

// 8x8x8 tiled-linear bit address and its inverse (VolumeRaytracer.cuh:107-171)
uint32_t GetSampleIndex(uint32_t x, uint32_t y, uint32_t z, uint32_t width, uint32_t height);
void GetPositionFromSampleIndex(uint32_t index, uint32_t width, uint32_t height, uint32_t& x, uint32_t& y, uint32_t& z);

template <class T>
struct Bounds {
    T min;
    T max;
};

template <typename T>
class RayTraceResults {  // VolumeRaytracer.cuh:179-202
public:
    std::shared_ptr<bool[]> valid{};
    std::shared_ptr<T[]> hitPoint{};
    std::shared_ptr<T[]> normal{};
    std::shared_ptr<float[]> distance{};
    std::shared_ptr<int[]> voxelIndex{};
    std::shared_ptr<int[]> steps{};
    explicit RayTraceResults(size_t count)
    {
        if (count == 0)
            return;
        valid = std::shared_ptr<bool[]>(new bool[count]());
        hitPoint = std::shared_ptr<T[]>(new T[count]());
        normal = std::shared_ptr<T[]>(new T[count]());
        distance = std::shared_ptr<float[]>(new float[count]());
        voxelIndex = std::shared_ptr<int[]>(new int[count]());
        steps = std::shared_ptr<int[]>(new int[count]());
    }
};

struct BitRef {  // VolumeRaytracer.cuh:204-209; writes are atomic RMW like the reference's
    uint32_t* byte = nullptr;
    size_t index = 0;
    operator bool() const;
    BitRef& operator=(bool value);
};

struct BitArray {  // VolumeRaytracer.cuh:210-223: LSB-first bits in u32 words
private:
    size_t size = 0;
    uint32_t* data = nullptr;

public:
    BitArray();
    BitArray(const BitArray& other, bool isGPU);  // deep copy to host (false) or device (true) memory
    BitArray(size_t num_bits, bool isGPU);
    BitArray(const BitArray&) = default;           // shallow, like the reference's implicit copy
    BitArray& operator=(const BitArray&) = default;
    bool operator[](size_t index) const;
    BitRef operator[](size_t index);
    uint32_t* Raw();
    const uint32_t* Raw() const;
    size_t BitSize() const;
    size_t ByteSize() const;
};
// prints every bit as 0/1, first bit first (VolumeRaytracer.cu:86-93); host arrays only
std::ostream& operator<<(std::ostream& os, const BitArray& bits);


template <size_t D>
struct VoxelBuffer {
    BitArray grid{};
    uint16_t dimensions[D]{};
};
typedef VoxelBuffer<3> VoxelBuffer3D;
typedef Bounds<float3> Bounds3Df;

constexpr size_t MAX_STEPS = 2048;

class VoxelRaytracer3D {  // VolumeRaytracer.cuh:291-377
    VoxelRaytracer3D(const VoxelRaytracer3D&) = delete;
    VoxelRaytracer3D& operator=(const VoxelRaytracer3D&) = delete;

public:
    explicit VoxelRaytracer3D(size_t count);
    ~VoxelRaytracer3D();
    void Free();

    void UploadVoxelBuffer(const VoxelBuffer3D& buff);
    void UploadVoxelBufferDatas(VoxelBuffer3D* buff, size_t count);
    void UploadVoxelBufferDataBounds(Bounds3Df* bounds, size_t count);
    int GetFactor() const { return factor; }
    void SetFactor(int f);
    // opaque: the device tables live behind the C ABI
    VoxelBuffer3D* GetVoxelBuffer() { return nullptr; }
    VoxelBuffer3D* GetVoxelBufferDatas() { return nullptr; }
    Bounds3Df* GetVoxelBufferDataBounds() { return nullptr; }

    RayTraceResults<float3> Raytrace(std::vector<float3> origin, std::vector<float3> ray);

    // facade extras
    vxrt_ctx* Context();        // uploads pending tables first
    // CreateVoxels + GenerateLowresVoxelBuffer + Upload* in one on-device step (no dense intermediate)
    void BuildProceduralWorld(uint3 size, int factor, int generator = 1);
    // voxel editing (an extension; the reference lists "Fully modifiable terrain" as to do, README.md:16): box / sphere
    // set and clear ops applied in order to the resident world (vxrt_edit_voxels); pending uploads are flushed first.
    // Return the vxrt_status of the call (0 = done; on failure the world is unchanged).
    int EditVoxels(const vxrt_edit_op* ops, size_t n, vxrt_edit_stats* stats = nullptr);
    int ReserveBricks(size_t capacity_bricks);  // grow the brick pool ahead of edits (vxrt_edit_reserve)
    // region readback and voxel stamps (extensions, include/vxrt.h): the voxels of the box origin .. origin + dims - 1 into
    // `bits` in the region layout (vxrt_read_region_host), and such a region written back at `origin` in a vxrt_stamp_mode
    // (vxrt_edit_stamps; the host words are copied to the device here).  Pending uploads are flushed first.  Return the
    // vxrt_status of the call (copy / paste: ReadRegion, then StampVoxels; undo: ReadRegion before an edit, then
    // StampVoxels with VXRT_STAMP_REPLACE).
    int ReadRegion(const int32_t origin[3], const int32_t dims[3], std::vector<uint32_t>& bits);
    int StampVoxels(const int32_t origin[3], const int32_t dims[3], const uint32_t* bits, int mode,
                    vxrt_edit_stats* stats = nullptr);
    // box collision queries (extensions, include/vxrt.h): n bodies moved axis by axis in `order` (a permutation of
    // {0, 1, 2}; y, x, z when NULL) and stopped at the first solid voxel each leading face would enter -- lohi_out gets
    // n x 6 floats (lo, hi), flags_or_null the VXRT_BODY_* bits (vxrt_move_boxes_host) -- and the solid voxels each body
    // overlaps (vxrt_overlap_boxes_host).  Host arrays; pending uploads are flushed first.  Return the vxrt_status.
    int MoveBoxes(const vxrt_body* bodies, size_t n, float* lohi_out, uint32_t* flags_or_null = nullptr,
                  const int32_t* order = nullptr);
    int OverlapBoxes(const vxrt_body* bodies, size_t n, uint32_t* counts, uint32_t* flags_or_null = nullptr);
    // floating islands (extension, include/vxrt.h, vxrt_find_islands_host): the island voxels of the box origin .. origin +
    // dims - 1 under the VXRT_ISLAND_ANCHOR_* bits `anchors` into `floating` (region words: a subtract stamp at origin
    // deletes them), the summary, and optionally the per-voxel component ids and up to max_islands table rows.  Pending
    // uploads are flushed first.  Returns the vxrt_status.
    int FindIslands(const int32_t origin[3], const int32_t dims[3], uint32_t anchors, std::vector<uint32_t>& floating,
                    vxrt_island_summary& summary, std::vector<vxrt_island>* islands = nullptr, uint32_t max_islands = 4096,
                    std::vector<uint32_t>* labels = nullptr);
    // voxel piece queries (extension, include/vxrt.h, vxrt_place_pieces_host): n placements of up to VXRT_PLACE_MAX_PIECES
    // rigid pieces against the resident world -- per placement the solid voxels overlapped at the origin, the travel along
    // one axis before the first overlap, the contact voxels and the VXRT_PLACED_* flags.  The pieces' d_bits are HOST words
    // here.  Pending uploads are flushed first.  Returns the vxrt_status.
    int PlacePieces(const vxrt_piece* pieces, size_t n_pieces, const vxrt_placement* placements, size_t n, vxrt_placed* results);
    // falling islands: the islands of the box origin .. origin + dims - 1 (FindIslands with labels) fall and land instead of
    // vanishing.  If the island table was cut short (more than max_islands islands) or an island's box exceeds the piece
    // limits, VXRT_ERR_INVALID before any change.  Otherwise one VXRT_STAMP_SUBTRACT stamp of the floating bits, then the
    // islands in ascending (lo[1], id): the island's piece is the bits of labels == id over its box lo .. hi, placed at lo with
    // axis 1 and dist = -min(lo[1], VXRT_PLACE_MAX_DIST), and written back with one VXRT_STAMP_UNION stamp at
    // lo + (0, travel, 0).  Later islands land on earlier ones: a deterministic sequential rule, not a physics engine; an
    // island that starts overlapping one that has already landed merges with it, and the cost is one synchronising edit per
    // island.  `rows` gets one {id, voxels, travel, contact} per island in dropping order.  Returns the vxrt_status.
    struct DroppedIsland {
        uint32_t id, voxels;
        int32_t travel;
        uint32_t contact;
    };
    int DropIslands(const int32_t origin[3], const int32_t dims[3], uint32_t anchors, std::vector<DroppedIsland>& rows,
                    uint32_t max_islands = 4096);
    // navigation fields (extension, include/vxrt.h, vxrt_nav_field_host): the walkable bits (region words), one next code
    // per cell and optionally the distances of the box origin .. origin + dims - 1 for `agent` toward the n_goals world
    // cells `goals` (3 int32 each), and the summary.  Pending uploads are flushed first.  Returns the vxrt_status.
    int NavField(const int32_t origin[3], const int32_t dims[3], const vxrt_nav_agent& agent, const int32_t* goals,
                 uint32_t n_goals, uint32_t max_dist, std::vector<uint32_t>& walkable, std::vector<uint8_t>& next,
                 vxrt_nav_summary& summary, std::vector<uint32_t>* dist = nullptr);
    // the paths of n start cells along the next codes of a NavField of the same box and agent (vxrt_nav_paths, through
    // device copies; synchronous): the moves made, the VXRT_NAV_* status and optionally the cells, max_steps + 1 per start
    int NavPaths(const int32_t origin[3], const int32_t dims[3], const vxrt_nav_agent& agent, const std::vector<uint8_t>& next,
                 const int32_t* starts, size_t n, uint32_t max_steps, std::vector<uint32_t>& lengths,
                 std::vector<uint32_t>& status, std::vector<int32_t>* cells = nullptr);
    // exact distance fields (extension, include/vxrt.h, vxrt_distance_field_host): the squared distance of every voxel of
    // the box origin .. origin + dims - 1 to the nearest VXRT_DIST_TO_SOLID / VXRT_DIST_TO_EMPTY voxel of the world within
    // `radius`, VXRT_DIST_FAR beyond it (one uint16 per voxel in region order), and the summary.  Pending uploads are flushed
    // first.  Returns the vxrt_status.
    int DistanceField(const int32_t origin[3], const int32_t dims[3], uint32_t radius, int32_t mode, std::vector<uint16_t>& dist2,
                      vxrt_distance_summary& summary);
    // mesh voxelization (extension, include/vxrt.h, vxrt_voxelize_mesh_host): `vertices` 3 int32 per vertex in units of
    // 1 / 256 voxel in the frame of a region of `dims` voxels, `triangles` 3 vertex indices per triangle, `modes` a subset of
    // VXRT_VOX_SURFACE | VXRT_VOX_SOLID; `bits` gets the region words (a StampVoxels argument as it is).  No world is needed.
    int VoxelizeMesh(const std::vector<int32_t>& vertices, const std::vector<uint32_t>& triangles, const int32_t dims[3],
                     int32_t modes, std::vector<uint32_t>& bits, vxrt_voxelize_summary& summary);
    // VoxelizeMesh into the mesh's own bounding box (the voxels its valid triangles' vertices touch, at most
    // VXRT_VOX_MAX_DIM per axis), then one StampVoxels of it in `stampMode`: mesh unit (0, 0, 0) lands on the corner of world
    // voxel `origin`.  Returns the vxrt_status; VXRT_ERR_INVALID for a mesh without a triangle of valid indices.
    int StampMesh(const std::vector<int32_t>& vertices, const std::vector<uint32_t>& triangles, const int32_t origin[3],
                  int32_t modes, int stampMode, vxrt_edit_stats* stats = nullptr, vxrt_voxelize_summary* summary = nullptr);
    // surface extraction (extension, include/vxrt.h, vxrt_extract_surface_host): the surface of the box `origin`, `dims` of
    // the resident world as merged quads in canonical order, `mode` VXRT_SURF_CAP or VXRT_SURF_OPEN; with `vertices` and
    // `triangles` (both or neither) also as a mesh in VoxelizeMesh's input format.  A counting call sizes the vectors, a
    // second call fills them.  Flushes queued edits first.  Returns the vxrt_status.
    int ExtractSurface(const int32_t origin[3], const int32_t dims[3], int32_t mode, std::vector<vxrt_quad>& quads,
                       vxrt_surface_summary* summary = nullptr, std::vector<int32_t>* vertices = nullptr,
                       std::vector<uint32_t>* triangles = nullptr);

    // occupancy LOD (extension, include/vxrt.h, vxrt_downsample_region_host): the box of `dims` cells of (1 << shift)^3 voxels
    // at world voxel `origin` reduced to one bit per cell, set when the cell holds at least `threshold` solid voxels (1 = any),
    // as region words (a stamp's bits for a coarser world); with `counts` also one uint16 per cell in region order.  Flushes
    // queued edits first.  Returns the vxrt_status.
    int DownsampleRegion(const int32_t origin[3], const int32_t dims[3], uint32_t shift, uint32_t threshold,
                         std::vector<uint32_t>& bits, vxrt_lod_summary& summary, std::vector<uint16_t>* counts = nullptr);

    // voxel light fields (extension, include/vxrt.h, vxrt_light_field_host): the sky and block light levels of every voxel of
    // the box origin .. origin + dims - 1, one byte (sky << 4) | block per voxel in region order, and the summary.
    // `emitters`: 4 int32 (x, y, z, level) per entry; `channels` a subset of VXRT_LIGHT_SKY | VXRT_LIGHT_BLOCK.  Flushes
    // queued edits first.  Returns the vxrt_status.
    int LightField(const int32_t origin[3], const int32_t dims[3], const std::vector<int32_t>& emitters, uint32_t channels,
                   std::vector<uint8_t>& levels, vxrt_light_summary& summary);

    // voxel materials (extension, include/vxrt.h, vxrt_material_field_host): the material byte of every voxel of the box
    // origin .. origin + dims - 1 in region order -- 0 for an empty voxel, else the paint byte or the strata rule -- and the
    // summary.  `paint`: one byte per voxel of rules.paint_origin / paint_dims in region order, or NULL.  Flushes queued edits
    // first.  Returns the vxrt_status.
    int MaterialField(const int32_t origin[3], const int32_t dims[3], const vxrt_material_rules& rules, std::vector<uint8_t>& materials,
                      vxrt_material_summary& summary, const uint8_t* paint = nullptr);

    // voxel rules (extension, include/vxrt.h, vxrt_apply_rule_host): the box origin .. origin + dims - 1 after the rule's
    // iterations as region words (a StampVoxels argument as it is) and the summary; the world is not changed.  `mask`:
    // region words of `dims` (VXRT_RULE_BOX only: the voxels a step may change) or NULL.  Flushes queued edits first.
    // Returns the vxrt_status.
    int ApplyRule(const int32_t origin[3], const int32_t dims[3], const vxrt_rule& rule, std::vector<uint32_t>& bits,
                  vxrt_rule_summary& summary, const uint32_t* mask = nullptr);
    // ApplyRule with the majority rule (N26, born with 14 or more solid neighbours, kept with 13 or more) on the box alone,
    // then one StampVoxels of the result in VXRT_STAMP_REPLACE: the box is smoothed in place.  Returns the vxrt_status.
    int SmoothVoxels(const int32_t origin[3], const int32_t dims[3], int32_t iterations = 1, vxrt_edit_stats* stats = nullptr,
                     vxrt_rule_summary* summary = nullptr);

    // loose voxels (extension, include/vxrt.h, vxrt_loose_step_host): the loose layer `loose` (region words of `dims`) of the
    // box origin .. origin + dims - 1 advanced by params.steps steps of falling, sliding and (water) spreading over the
    // world's solids, in place, and the summary; the world is not changed.  Flushes queued edits first.  Returns the
    // vxrt_status.
    int StepLoose(const int32_t origin[3], const int32_t dims[3], const vxrt_loose& params, std::vector<uint32_t>& loose,
                  vxrt_loose_summary& summary);
    // The solid voxels of the source box, which must lie inside the box, turned loose and settled: lifted out of the world
    // (VXRT_STAMP_SUBTRACT), stepped with StepLoose in calls of at most VXRT_LOOSE_MAX_STEPS steps with the phase carried
    // until a call's last step neither drops nor slides a voxel (`early_stop`) or max_steps steps are made, and stamped back
    // with VXRT_STAMP_UNION.  *steps: the steps made.  Returns the vxrt_status.
    int SettleVoxels(const int32_t origin[3], const int32_t dims[3], const int32_t source_origin[3], const int32_t source_dims[3],
                     int32_t material, int32_t max_steps, int32_t edge, vxrt_loose_summary* summary = nullptr,
                     int32_t* steps = nullptr, vxrt_edit_stats* stats = nullptr, bool early_stop = true);

private:
    void Flush();
    vxrt_ctx* ctx = nullptr;
    int factor = 1;
    bool dirty = false;
    uint16_t cdims[3] = {0, 0, 0};
    std::vector<uint32_t> coarse_bits, brick_slot, pool;
    std::vector<float> bounds;
    bool have_coarse = false, have_bricks = false, have_bounds = false;
};

// Brickmap build on host threads (VolumeRaytracer.cuh:379-516).  Returned arrays are heap-owned by the caller,
// as in the reference; empty bricks have dimensions 0 and no bits.
std::tuple<VoxelBuffer3D, VoxelBuffer3D*, Bounds3Df*> GenerateLowresVoxelBuffer(const VoxelBuffer3D& originalData, int factor);

}  // namespace GPUDDA
