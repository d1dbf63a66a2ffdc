// vxrt_api.hip -- host side of the C ABI declared in include/vxrt.h.
// Owns the HBM-resident world tables, the camera/lighting state the reference keeps in
// process globals (hFrameInfo / g_env, VoxelRT/Renderer.cu:24-25,89) and the launches.
#include "../../include/vxrt.h"
#include "vxrt_denoise.hpp"
#include "vxrt_dist.hpp"
#include "vxrt_light.hpp"
#include "vxrt_edit.hpp"
#include "vxrt_kernels.hpp"
#include "vxrt_islands.hpp"
#include "vxrt_lod.hpp"
#include "vxrt_nav.hpp"
#include "vxrt_place.hpp"
#include "vxrt_region.hpp"
#include "vxrt_stream.hpp"
#include "vxrt_surface.hpp"
#include "vxrt_voxelize.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <new>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace vxrt {
hipError_t launch_render(const RenderArgs& A, bool stats, int variant, hipStream_t stream);
int resolve_render_variant(const RenderArgs& A, int variant);
bool launch_is_common(const RenderArgs& A);
hipError_t launch_trace_batch(const BatchArgs& B, bool stats, int variant, hipStream_t stream);
void launch_deinterleave(const void* shards, unsigned long long shard_stride_bytes, void* fb, uint32_t width,
                         uint32_t height, uint32_t strip_rows, uint32_t strip_count, hipStream_t stream, uint32_t n_views = 1,
                         unsigned long long view_stride_bytes = 0, unsigned long long fb_stride_bytes = 0);
int build_world_on_device(struct ::vxrt_ctx* ctx, int generator, int X, int Y, int Z, int factor);
// re-ordering between the reference's tiled bit order (the C ABI's and the file's) and the HBM order (vxrt_worldgen.hip)
hipError_t layout_bits(const uint32_t* src, uint32_t* dst, const int cd[3], bool to_hbm);
hipError_t layout_meta(const uint2* src, uint2* dst, const int cd[3], bool to_hbm);
hipError_t layout_bricks(const uint32_t* src, uint32_t* dst, uint64_t nbricks, int f, bool to_hbm);  // src == dst: in place
hipError_t chunk_tables(uint2* meta, uint32_t* coarse, const uint2* d_chunk_meta, int tx, int ty, int tz, int cx, int cz);
// voxel editing (vxrt_edit.hip)
hipError_t edit_bricks(const uint32_t* cells, uint32_t n, const EditOpDev* ops, uint32_t nops, const uint2* meta,
                       const uint32_t* pool, uint32_t* scratch, uint32_t* ext, uint2* info, int f, int cx, int cz);
hipError_t edit_commit(const uint32_t* cells, const uint32_t* new_slot, uint32_t n, const uint32_t* zero, uint32_t nzero,
                       const uint32_t* scratch, const uint32_t* ext, uint32_t* pool, uint2* meta, uint32_t* coarse, int f);
hipError_t gather_bricks(const uint32_t* pool, const uint32_t* idx, uint32_t n, uint32_t* dst, int f);
// voxel stamps (vxrt_region.hip; read_region: vxrt_region.hpp)
hipError_t stamp_bricks(const uint32_t* cells, uint32_t n, const StampDev* stamps, uint32_t nst, const uint2* meta,
                        const uint32_t* pool, uint32_t* scratch, uint32_t* ext, uint2* info, int f, int cx, int cz);
// box collision queries (vxrt_collide.hip)
hipError_t move_boxes(const CollideWorld& W, const float* bodies, uint64_t n, const int order[3], float* lohi, uint32_t* flags,
                      hipStream_t stream);
hipError_t overlap_boxes(const CollideWorld& W, const float* bodies, uint64_t n, uint32_t* counts, uint32_t* flags,
                         hipStream_t stream);
// floating islands (vxrt_islands.hip)
hipError_t find_islands(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t anchors, void* work,
                        uint32_t* floating, uint32_t* labels, vxrt_island* table, uint32_t max_islands,
                        vxrt_island_summary* summary, hipStream_t stream);
// voxel piece queries (vxrt_place.hip)
hipError_t place_pieces(const PlaceArgs& A, hipStream_t stream);
// navigation fields (vxrt_nav.hip)
hipError_t nav_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], const vxrt_nav_agent& ag, const int32_t* goals,
                     uint32_t ngoals, uint32_t max_dist, void* work, uint32_t* walkable, uint8_t* next, uint32_t* dist,
                     vxrt_nav_summary* summary, hipStream_t stream);
hipError_t nav_paths(const NavPathArgs& P, hipStream_t stream);
// light fields (vxrt_light.hip)
hipError_t light_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t channels, const int32_t* emitters,
                       uint32_t n_emitters, void* work, uint8_t* levels, vxrt_light_summary* summary, hipStream_t stream);
// distance fields (vxrt_dist.hip)
hipError_t distance_field(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t radius, uint32_t mode, void* work,
                          uint16_t* dist2, vxrt_distance_summary* summary, hipStream_t stream);
// mesh voxelization (vxrt_voxelize.hip)
hipError_t voxelize_mesh(const int32_t* verts, uint32_t nv, const uint32_t* tris, uint32_t nt, const int32_t d[3], uint32_t modes,
                         void* work, uint32_t* bits, vxrt_voxelize_summary* summary, uint32_t work_waves, hipStream_t stream);
// surface extraction (vxrt_surface.hip)
hipError_t extract_surface(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t mode, void* work, vxrt_quad* quads,
                           uint32_t capacity, int32_t* verts, uint32_t* tris, vxrt_surface_summary* summary, hipStream_t stream);
// occupancy LOD (vxrt_lod.hip)
hipError_t frame_guides(const RenderArgs& R, uint32_t Z, uint32_t* keys, hipStream_t stream);
hipError_t denoise_frame(uint32_t W, uint32_t H, const float* color_in, const uint32_t* keys, int32_t iterations, float k,
                         void* work, float* color_out, void* fb, hipStream_t stream);
hipError_t downsample_region(const CollideWorld& W, const int32_t o[3], const int32_t d[3], uint32_t shift, uint32_t threshold,
                             void* work, uint32_t* bits, uint16_t* counts, vxrt_lod_summary* summary, hipStream_t stream);
}  // namespace vxrt

static thread_local std::string g_last_error = "";

static int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

#define VX_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(VXRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));              \
    } while (0)

struct vxrt_ctx {
    int device = 0;
    // world
    bool has_world = false;
    vxrt::WorldView view{};
    uint32_t* d_coarse = nullptr;   // (inside coarse_alloc, with slack before and behind: vxrt_wave2.hpp)
    void* coarse_alloc = nullptr;
    void* pool_alloc = nullptr;
    uint2* d_meta = nullptr;
    uint32_t* d_pool = nullptr;
    uint64_t ncells = 0, nslots = 0, pool_capacity_slots = 0;
    uint64_t coarse_alloc_bytes = 0, pool_alloc_bytes = 0;  // what is addressable around the two bit tables (load guard)
    bool guard_no_slack = false;  // vxrt_debug_guard_pretend_no_slack
    // state the reference keeps in globals
    float light_dir[3] = {0, 0, 0};  // g_env is a zero-initialised device global until SetEnvironment (Renderer.cu:89)
    float light_color[3] = {0, 0, 0};
    float ambient[3] = {0, 0, 0};
    float fov = 90.0f;               // hFrameInfo initial value, Renderer.cu:25
    float ortho[2] = {10.0f, 10.0f};
    uint32_t frame_counter = 0;
    int kernel_variant = 4;          // 4 = default (= 7: the persistent kernels on the tracer of vxrt_wave2.hpp), 1 = straightforward loops
    unsigned persistent_waves = 4096;
    unsigned cus = 256;
    unsigned long long* d_stats = nullptr;
    unsigned int* d_queues = nullptr;  // kTileCounterRing queue heads of vxrt::kQueueWords words (one per launch in flight)
    // Counters only ever grow on the device (atomics from any stream); "read and clear" is a host-side snapshot that the
    // next read subtracts, so nothing clears device memory under running kernels.
    unsigned long long stats_base[vxrt::kStatCount] = {};
    // Rings: queue heads (render tile counters / batch tickets) and per-view argument slots of multi-view launches.  A ring
    // entry carries the event of the launch that used it last; taking an entry that is still in flight waits for that launch
    // (launch 65 of 64 in flight, multi-view launch 17 of 16), so an entry is never shared by two live launches.
    std::atomic<unsigned> launch_seq{0};
    hipEvent_t counter_busy[64] = {};
    vxrt::ViewArgs* d_views = nullptr;
    std::atomic<unsigned> view_seq{0};
    hipEvent_t views_busy[16] = {};
    int batch_max_steps = vxrt::kMaxSteps;  // Raytrace's maxSteps for the batch API (vxrt_set_batch_max_steps)
    struct StreamState* stream = nullptr;   // chunk streaming (vxrt_stream_*), or NULL
    // voxel editing (vxrt_edit_voxels): slots below nslots that hold no brick, and whether an edit has changed the world
    // since it was made resident (vxrt_save_world then compacts the pool)
    std::set<uint32_t> free_slots;
    bool edited = false;
    struct DevBuf {  // grow-only device scratch of the edit calls
        void* p = nullptr;
        size_t bytes = 0;
        hipError_t reserve(size_t n)
        {
            if (n <= bytes)
                return hipSuccess;
            (void)hipFree(p);
            p = nullptr;
            bytes = 0;
            hipError_t e = hipMalloc(&p, n);
            if (e == hipSuccess)
                bytes = n;
            return e;
        }
        void release() { (void)hipFree(p); p = nullptr; bytes = 0; }
    } edit_in, edit_scratch, edit_out, edit_plan;
};
constexpr unsigned kViewSlots = 16;  // multi-view launches that may be in flight at once on one context
constexpr unsigned kTileCounterRing = 64;  // render launches that may be in flight at once on one context
static_assert(kTileCounterRing == sizeof(vxrt_ctx::counter_busy) / sizeof(hipEvent_t), "ring size");
static_assert(kViewSlots == sizeof(vxrt_ctx::views_busy) / sizeof(hipEvent_t), "ring size");

namespace vxrt {

void stream_drop(vxrt_ctx* c);  // defined with the chunk streaming code below

static void free_world(vxrt_ctx* c)
{
    stream_drop(c);
    if (c->coarse_alloc) (void)hipFree(c->coarse_alloc);
    if (c->d_meta) (void)hipFree(c->d_meta);
    if (c->pool_alloc) (void)hipFree(c->pool_alloc);
    c->coarse_alloc = c->pool_alloc = nullptr;
    c->d_coarse = nullptr;
    c->d_meta = nullptr;
    c->d_pool = nullptr;
    c->has_world = false;
    c->ncells = c->nslots = c->pool_capacity_slots = 0;
    c->free_slots.clear();
    c->edited = false;
}

// shared by upload and the device builder
int check_shape(int factor, const int cd[3])
{
    if (!(factor == 8 || factor == 16 || factor == 32))
        return fail(VXRT_ERR_INVALID, "factor must be 8, 16 or 32");
    for (int a = 0; a < 3; ++a)
        if (cd[a] <= 0 || cd[a] % 8 != 0 || cd[a] > 65535)
            return fail(VXRT_ERR_INVALID, "coarse dimensions must be positive multiples of 8 (the tables' tiled order)");
    // cell_index(): x + cx * (z + cz * y) by two 24-bit multiply-adds, 32-bit bit indices biased by one x-z slice, and a
    // lane that has just left the grid may look one more slice ahead (vxrt_wave2.hpp)
    const uint64_t slice = (uint64_t)cd[0] * (uint64_t)cd[2];
    if ((uint64_t)cd[1] * (uint64_t)cd[2] >= (1ull << 24) || slice * (uint64_t)cd[1] + 2ull * slice + 64ull >= (1ull << 32))
        return fail(VXRT_ERR_INVALID, "coarse grid too large for 32-bit cell indices (cy * cz must stay below 2^24, cx * cz * (cy + 2) below 2^32)");
    return VXRT_OK;
}

void fill_view(vxrt_ctx* c, int factor, const int cd[3])
{
    WorldView& v = c->view;
    v.coarse_bits = c->d_coarse;
    v.cell_meta = c->d_meta;
    v.pool = c->d_pool;
    v.cx = cd[0];
    v.cy = cd[1];
    v.cz = cd[2];
    v.c_row = cd[0];
    v.c_slice = cd[0] * cd[2];
    v.f = factor;
    v.f_row = factor;
    v.f_slice = factor * factor;
    v.brick_words = (uint32_t)(factor * factor * factor / 32);
    v.ff = (float)factor;
    v.inv_f = 1.0f / (float)factor;
    v.wmax_x = (float)((double)cd[0] - 1e-6);  // dims - FLT_EPS_DDA in double, VolumeRaytracer.cu:375-376
    v.wmax_y = (float)((double)cd[1] - 1e-6);
    v.wmax_z = (float)((double)cd[2] - 1e-6);
    v.X = cd[0] * factor;
    v.Y = cd[1] * factor;
    v.c_wide = grid_is_wide(cd[0], cd[1], cd[2]) ? 1 : 0;
    // load guard of the probe-counting kernels: the tables proper, and the allocations around them
    v.coarse_end = c->d_coarse + (c->ncells + 31) / 32;
    v.pool_end = c->d_pool + (c->pool_capacity_slots ? c->pool_capacity_slots : 1) * (uint64_t)v.brick_words;
    v.coarse_lo = c->guard_no_slack ? v.coarse_bits : static_cast<const uint32_t*>(c->coarse_alloc);
    v.coarse_hi = c->guard_no_slack ? v.coarse_end : v.coarse_lo + c->coarse_alloc_bytes / 4;
    v.pool_lo = c->guard_no_slack ? v.pool : static_cast<const uint32_t*>(c->pool_alloc);
    v.pool_hi = c->guard_no_slack ? v.pool_end : v.pool_lo + c->pool_alloc_bytes / 4;
}

// The pool's allocation: `slots` bricks of `bw` words (at least one), behind and followed by one brick of addressable slack
// (the tracer's one load beyond a table, below).  Shared by every world path and the edit's pool growth.
static hipError_t alloc_pool(uint64_t bw, uint64_t slots, void** alloc, uint64_t* alloc_bytes, uint32_t** pool)
{
    const uint64_t pool_bytes = (slots ? slots : 1) * bw * sizeof(uint32_t);
    const uint64_t pool_slack = (bw * sizeof(uint32_t) + 255) / 256 * 256;
    hipError_t e = hipMalloc(alloc, pool_bytes + 2 * pool_slack);
    if (e != hipSuccess)
        return e;
    *alloc_bytes = pool_bytes + 2 * pool_slack;
    *pool = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(*alloc) + pool_slack);
    return hipSuccess;
}

int alloc_world(vxrt_ctx* c, int factor, const int cd[3], uint64_t pool_slots)
{
    free_world(c);
    c->ncells = (uint64_t)cd[0] * cd[1] * cd[2];
    uint64_t bw = (uint64_t)factor * factor * factor / 32;
    // The tracer of vxrt_wave2.hpp lets a lane that has just left the grid (or a brick) issue one more load, one x-z slice
    // (one brick row-plane) beyond the table at most: both tables sit inside allocations with that much addressable slack
    // before and behind them.  The slack is never written and its bits are never used.
    const uint64_t coarse_bytes = ((c->ncells + 31) / 32) * sizeof(uint32_t);
    const uint64_t coarse_slack = (((uint64_t)cd[0] * cd[2] / 8 + 64) + 255) / 256 * 256;
    VX_HIP(hipMalloc(&c->coarse_alloc, coarse_bytes + 2 * coarse_slack));
    c->coarse_alloc_bytes = coarse_bytes + 2 * coarse_slack;
    c->d_coarse = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(c->coarse_alloc) + coarse_slack);
    VX_HIP(hipMalloc((void**)&c->d_meta, c->ncells * sizeof(uint2)));
    VX_HIP(alloc_pool(bw, pool_slots, &c->pool_alloc, &c->pool_alloc_bytes, &c->d_pool));
    c->pool_capacity_slots = pool_slots;
    return VXRT_OK;
}

int adopt_world(vxrt_ctx* c, int factor, const int cd[3], uint64_t nslots, uint32_t** d_coarse, uint2** d_meta,
                uint32_t** d_pool)
{
    int rc = alloc_world(c, factor, cd, nslots);
    if (rc)
        return rc;
    c->nslots = nslots;
    fill_view(c, factor, cd);
    c->has_world = true;
    *d_coarse = c->d_coarse;
    *d_meta = c->d_meta;
    *d_pool = c->d_pool;
    return VXRT_OK;
}

int set_error(int code, const char* msg) { return fail(code, msg); }
void abandon_world(vxrt_ctx* c) { free_world(c); }

// Whether `stream` is being captured into a graph (include/vxrt.h, "Stream capture"); asked once per call.  The NULL
// stream is never asked: it cannot be captured, and asking while another stream captures is itself an error.
static bool stream_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &cs) != hipSuccess)
        (void)hipGetLastError();
    return cs != hipStreamCaptureStatusNone;
}

// Take ring entry `i`: if the launch that used it last has not finished, wait for it (the documented in-flight limits are
// enforced here instead of silently sharing a queue head).  Inside a stream capture nothing can be waited for or
// recorded: the capturing caller keeps within the limits itself.
static hipError_t ring_acquire(hipEvent_t& ev, bool capturing)
{
    if (capturing || !ev)
        return hipSuccess;
    hipError_t e = hipEventQuery(ev);
    if (e == hipErrorNotReady)
        e = hipEventSynchronize(ev);
    return e;
}

static hipError_t ring_release(hipEvent_t& ev, hipStream_t stream, bool capturing)
{
    if (capturing)
        return hipSuccess;
    if (!ev) {
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess)
            return e;
    }
    return hipEventRecord(ev, stream);
}

// One view's arguments stored to its place in a device view slot: what a CAPTURED multi-view launch issues instead of the
// copy from host memory.  Kernel arguments are copied into the graph's node, so every replay writes what the capture
// saw and reads no host memory (a captured hipMemcpyAsync keeps the host pointer).  One lane, about 1.1 KB.
__global__ void k_store_view(ViewArgs v, ViewArgs* dst)
{
    if (threadIdx.x == 0)
        *dst = v;
}

// Default hand-out order of the persistent kernel's tile queue: expected-longest ray chains first, so that what is
// still in flight when the queue runs dry is cheap.  The cost proxy needs the camera only: the elevation of the
// centre ray of each 8-pixel tile row in a Y-up world -- rays just below the horizon travel farthest, rays
// pointing up leave the grid at once.  A few hundred flops on the host per frame; scheduling only.
static void schedule_tile_rows(const RenderArgs& A, const f3& fwd, const f3& up, uint16_t* order, uint32_t& order_n)
{
    const unsigned nty = (A.launch_rows + 7u) / 8u;
    order_n = 0;
    if (nty < 2 || nty > kMaxScheduledTileRows)
        return;
    std::vector<std::pair<float, uint16_t>> key(nty);
    for (unsigned j = 0; j < nty; ++j) {
        unsigned row = j * 8u + 4u < A.launch_rows ? j * 8u + 4u : A.launch_rows - 1u;
        unsigned y = row;  // launch row -> frame row (pixel_coords in vxrt_persist2.hpp)
        if (A.checkerboard)
            y = 2u * row;
        else if (A.strip_count > 1)
            y = ((row / (unsigned)A.strip_rows) * (unsigned)A.strip_count + (unsigned)A.strip_index) * (unsigned)A.strip_rows +
                row % (unsigned)A.strip_rows;
        const float sv = ((float)y / (float)A.height) * 2.0f - 1.0f;
        float dy = fwd.y;
        if (!A.ortho) {
            const float dx = fwd.x + sv * A.ky * up.x, dz = fwd.z + sv * A.ky * up.z;
            dy = fwd.y + sv * A.ky * up.y;
            const float len = sqrtf(dx * dx + dy * dy + dz * dz);
            dy = len > 0.0f ? dy / len : dy;
        }
        key[j] = {dy < 0.0f ? -dy : 2.0f + dy, (uint16_t)j};  // grazing-down first ... straight down, then up
    }
    std::stable_sort(key.begin(), key.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (unsigned j = 0; j < nty; ++j)
        order[j] = key[j].second;
    order_n = nty;
}

}  // namespace vxrt

extern "C" {

int vxrt_abi_version(void) { return VXRT_ABI_VERSION; }

const char* vxrt_last_error(void) { return g_last_error.c_str(); }

int vxrt_create(int device, vxrt_ctx** out)
{
    if (!out)
        return fail(VXRT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    VX_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(VXRT_ERR_INVALID, "no such HIP device");
    VX_HIP(hipSetDevice(device));
    vxrt_ctx* c = new (std::nothrow) vxrt_ctx();
    if (!c)
        return fail(VXRT_ERR_NOMEM, "out of host memory");
    c->device = device;
    // counters, and a ring of queue heads for the persistent kernels: launches on different streams may be in flight
    // together (frame k+1 fills the SIMD slots frame k's last waves leave), each needs its own queue head
    const size_t stat_words = (size_t)vxrt::kStatRows * vxrt::kStatRowStride;  // (vxrt_kernels.hpp: rows of counters)
    hipError_t e = hipMalloc((void**)&c->d_stats, stat_words * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemset(c->d_stats, 0, stat_words * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMalloc((void**)&c->d_queues, sizeof(unsigned int) * vxrt::kQueueWords * kTileCounterRing);
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, device);
        c->persistent_waves = (unsigned)prop.multiProcessorCount * 16u;  // 4 waves per SIMD at <= 128 VGPRs
        c->cus = (unsigned)prop.multiProcessorCount;
#ifdef VXRT_EXPERIMENTS  // A/B builds only (make libvxrt_exp.so): the product library reads no environment variable
        if (const char* e = getenv("VXRT_WAVES_PER_CU"))                  // occupancy / grid experiments
            if (atoi(e) > 0 && atoi(e) <= 32)
                c->persistent_waves = (unsigned)prop.multiProcessorCount * (unsigned)atoi(e);
#endif
    }
    if (e != hipSuccess) {
        if (c->d_stats) (void)hipFree(c->d_stats);
        if (c->d_queues) (void)hipFree(c->d_queues);
        delete c;
        return fail(VXRT_ERR_HIP, std::string("context setup: ") + hipGetErrorString(e));
    }
    *out = c;
    return VXRT_OK;
}

int vxrt_destroy(vxrt_ctx* c)
{
    if (!c)
        return VXRT_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    vxrt::free_world(c);
    if (c->d_stats) (void)hipFree(c->d_stats);
    if (c->d_queues) (void)hipFree(c->d_queues);
    if (c->d_views) (void)hipFree(c->d_views);
    c->edit_in.release();
    c->edit_scratch.release();
    c->edit_out.release();
    c->edit_plan.release();
    for (hipEvent_t& e : c->counter_busy)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t& e : c->views_busy)
        if (e) (void)hipEventDestroy(e);
    delete c;
    return VXRT_OK;
}

int vxrt_kernel_for_launch(const vxrt_ctx* c, uint32_t width, uint32_t height, const vxrt_render_flags* fl, uint32_t nviews)
{
    if (!c || !fl || fl->struct_size != sizeof(vxrt_render_flags))
        return -1;
    vxrt::RenderArgs A;
    memset(&A, 0, sizeof(A));
    if (c->has_world)
        A.W = c->view;
    A.width = width;
    A.shadow = fl->shadow ? 1 : 0;
    A.bounce_samples = fl->bounce_samples;
    A.nviews = nviews;
    // the launch grid's rows, as vxrt_render works them out
    if (fl->checkerboard)
        A.launch_rows = height >> 1;
    else if (fl->strip_count > 1)
        A.launch_rows = vxrt_compact_rows(height, fl->strip_rows > 0 ? fl->strip_rows : 16, fl->strip_count, fl->strip_index);
    else
        A.launch_rows = height;
    return vxrt::resolve_render_variant(A, c->kernel_variant);
}

int vxrt_render_specialisation(const vxrt_ctx* c, uint32_t width, uint32_t height, const vxrt_render_flags* fl, uint32_t nviews)
{
    if (!c || !fl || fl->struct_size != sizeof(vxrt_render_flags))
        return -1;
    (void)width;
    (void)height;
    if (!c->has_world || c->kernel_variant == 1)
        return 0;
    // the arguments launch_is_common reads, as vxrt_render_views fills them in
    vxrt::RenderArgs A;
    memset(&A, 0, sizeof(A));
    A.W = c->view;
    A.mode = fl->mode;
    A.checkerboard = fl->checkerboard ? 1 : 0;
    A.ortho = fl->ortho ? 1 : 0;
    A.strip_count = fl->strip_count > 1 ? fl->strip_count : 1;
    A.compact = fl->compact ? 1 : 0;
    A.accum = reinterpret_cast<float4*>(fl->d_accum);
    A.nviews = nviews;
    A.hit_aov = (long long*)fl->d_hit_aov;
    A.want_hit_aov = fl->d_hit_aov != nullptr;
    return vxrt::launch_is_common(A) ? 1 : 0;
}

int vxrt_set_persistent_waves_per_cu(vxrt_ctx* c, int waves_per_cu)
{
    if (!c || waves_per_cu < 0 || waves_per_cu > 32)
        return fail(VXRT_ERR_INVALID, "waves_per_cu must be in [1, 32], or 0 for the default");
    c->persistent_waves = c->cus * (unsigned)(waves_per_cu == 0 ? 16 : waves_per_cu);
    return VXRT_OK;
}

int vxrt_has_experiments(void)
{
#ifdef VXRT_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

int vxrt_debug_guard_pretend_no_slack(vxrt_ctx* c, int on)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "NULL context");
    c->guard_no_slack = on != 0;
    if (c->has_world) {
        const int cd[3] = {c->view.cx, c->view.cy, c->view.cz};
        vxrt::fill_view(c, c->view.f, cd);
    }
    return VXRT_OK;
}

int vxrt_set_kernel_variant(vxrt_ctx* c, int variant)
{
    if (!c || !(variant == 1 || variant == 4 || variant == 7))
        return fail(VXRT_ERR_INVALID, "variant must be 4 (default), 7 (the persistent kernels on the wave-level tracer: what the default runs) or 1 (straightforward per-lane loops, the cross-check)");
    c->kernel_variant = variant;
    return VXRT_OK;
}

int vxrt_synchronize(vxrt_ctx* c)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

int vxrt_upload_world(vxrt_ctx* c, const vxrt_world_desc* d)
{
    if (!c || !d || d->struct_size != sizeof(vxrt_world_desc))
        return fail(VXRT_ERR_INVALID, "bad ctx/desc");
    if (!d->coarse_bits || !d->brick_slot || !d->bounds || (d->nslots && !d->pool))
        return fail(VXRT_ERR_INVALID, "NULL table");
    int cd[3] = {d->cdims[0], d->cdims[1], d->cdims[2]};
    int rc = vxrt::check_shape(d->factor, cd);
    if (rc)
        return rc;
    VX_HIP(hipSetDevice(c->device));
    const int f = d->factor;
    const uint64_t ncells = (uint64_t)cd[0] * cd[1] * cd[2];
    // flatten {descriptor, bounds} pairs into 8-byte cell_meta records
    std::vector<uint2> meta(ncells);
    for (uint64_t i = 0; i < ncells; ++i) {
        bool bit = (d->coarse_bits[i >> 5] >> (i & 31)) & 1u;
        uint32_t slot = d->brick_slot[i];
        const float* b = d->bounds + i * 6;
        uint32_t packed = 0;
        if (bit) {
            if (slot == VXRT_EMPTY_SLOT || slot >= d->nslots)
                return fail(VXRT_ERR_INVALID, "occupied coarse cell without a valid brick slot");
            for (int k = 0; k < 6; ++k) {
                float v = b[k];
                if (!(v >= 0.0f && v <= (float)(f - 1) && v == (float)(int)v))
                    return fail(VXRT_ERR_INVALID, "brick extents must be integers in [0, factor-1]");
                packed |= (uint32_t)(int)v << (5 * k);
            }
        } else {
            slot = VXRT_EMPTY_SLOT;
        }
        meta[i] = make_uint2(slot, packed);
    }
    rc = vxrt::alloc_world(c, f, cd, d->nslots);
    if (rc)
        return rc;
    const uint64_t bw = (uint64_t)f * f * f / 32;
    // the tables arrive in the reference's tiled order and are re-ordered on the device into the HBM order
    const uint64_t coarse_bytes = ((ncells + 31) / 32) * sizeof(uint32_t);
    uint32_t* t_coarse = nullptr;
    uint2* t_meta = nullptr;
    hipError_t e = hipMalloc((void**)&t_coarse, coarse_bytes);
    if (e == hipSuccess)
        e = hipMalloc((void**)&t_meta, ncells * sizeof(uint2));
    if (e == hipSuccess)
        e = hipMemcpy(t_coarse, d->coarse_bits, coarse_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(t_meta, meta.data(), ncells * sizeof(uint2), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = vxrt::layout_bits(t_coarse, c->d_coarse, cd, true);
    if (e == hipSuccess)
        e = vxrt::layout_meta(t_meta, c->d_meta, cd, true);
    if (e == hipSuccess && d->nslots)
        e = hipMemcpy(c->d_pool, d->pool, d->nslots * bw * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && d->nslots)
        e = vxrt::layout_bricks(c->d_pool, c->d_pool, d->nslots, f, true);
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    (void)hipFree(t_coarse);
    (void)hipFree(t_meta);
    if (e != hipSuccess) {
        vxrt::free_world(c);
        return fail(VXRT_ERR_HIP, std::string("world upload: ") + hipGetErrorString(e));
    }
    c->nslots = d->nslots;
    vxrt::fill_view(c, f, cd);
    c->has_world = true;
    return VXRT_OK;
}

int vxrt_build_world_procedural(vxrt_ctx* c, int generator, int X, int Y, int Z, int factor)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    VX_HIP(hipSetDevice(c->device));
    return vxrt::build_world_on_device(c, generator, X, Y, Z, factor);
}

int vxrt_world_info_get(vxrt_ctx* c, vxrt_world_info* out)
{
    if (!c || !out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    out->factor = c->view.f;
    out->cdims[0] = c->view.cx;
    out->cdims[1] = c->view.cy;
    out->cdims[2] = c->view.cz;
    out->ncells = c->ncells;
    out->nslots = c->nslots;
    out->hbm_bytes = ((c->ncells + 31) / 32) * 4 + c->ncells * sizeof(uint2) + c->nslots * c->view.brick_words * 4ull;
    return VXRT_OK;
}

int vxrt_download_world(vxrt_ctx* c, uint32_t* coarse_bits, uint32_t* brick_slot, float* bounds, uint32_t* pool)
{
    if (!c || !coarse_bits || !brick_slot || !bounds)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());
    // back into the reference's tiled order, through device temporaries (the pool in pieces of at most 64 MiB)
    const int cd[3] = {c->view.cx, c->view.cy, c->view.cz};
    const uint64_t coarse_bytes = ((c->ncells + 31) / 32) * sizeof(uint32_t);
    const uint64_t bw = c->view.brick_words;
    const uint64_t piece = std::max<uint64_t>(1, (64ull << 20) / (bw * 4));  // bricks per piece
    uint32_t *t_coarse = nullptr, *t_pool = nullptr;
    uint2* t_meta = nullptr;
    std::vector<uint2> meta(c->ncells);
    hipError_t e = hipMalloc((void**)&t_coarse, coarse_bytes);
    if (e == hipSuccess)
        e = hipMalloc((void**)&t_meta, c->ncells * sizeof(uint2));
    if (e == hipSuccess)
        e = vxrt::layout_bits(c->d_coarse, t_coarse, cd, false);
    if (e == hipSuccess)
        e = vxrt::layout_meta(c->d_meta, t_meta, cd, false);
    if (e == hipSuccess)
        e = hipMemcpy(coarse_bits, t_coarse, coarse_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(meta.data(), t_meta, c->ncells * sizeof(uint2), hipMemcpyDeviceToHost);
    if (e == hipSuccess && pool && c->nslots) {
        e = hipMalloc((void**)&t_pool, std::min<uint64_t>(piece, c->nslots) * bw * 4);
        for (uint64_t at = 0; e == hipSuccess && at < c->nslots; at += piece) {
            const uint64_t n = std::min<uint64_t>(piece, c->nslots - at);
            e = vxrt::layout_bricks(c->d_pool + at * bw, t_pool, n, c->view.f, false);
            if (e == hipSuccess)
                e = hipMemcpy(pool + at * bw, t_pool, n * bw * 4, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(t_coarse);
    (void)hipFree(t_meta);
    (void)hipFree(t_pool);
    if (e != hipSuccess)
        return fail(VXRT_ERR_HIP, std::string("world download: ") + hipGetErrorString(e));
    for (uint64_t i = 0; i < c->ncells; ++i) {
        brick_slot[i] = meta[i].x;
        float* b = bounds + i * 6;
        if (meta[i].x == VXRT_EMPTY_SLOT) {
            b[0] = b[1] = b[2] = 0.0f;
            b[3] = b[4] = b[5] = -1.0f;  // VolumeRaytracer.cuh:454-467
        } else {
            for (int k = 0; k < 6; ++k)
                b[k] = (float)((meta[i].y >> (5 * k)) & 31u);
        }
    }
    return VXRT_OK;
}

int vxrt_set_environment(vxrt_ctx* c, const float light_dir[3], const float light_color[3], const float ambient[3])
{
    if (!c || !light_dir || !light_color || !ambient)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    {   // a light whose unit vector (the shadow rays' direction, unit3 of the launch set-up) is not a finite vector: every
        // shadow ray would be invalid (include/vxrt.h)
        const float lx = light_dir[0], ly = light_dir[1], lz = light_dir[2];
        const float dd = lx * lx + ly * ly + lz * lz;
        if (!std::isfinite(lx) || !std::isfinite(ly) || !std::isfinite(lz) || !(dd > 0.0f) || !std::isfinite(dd))
            return fail(VXRT_ERR_INVALID, "light_dir must be finite with a binary32 squared length that is positive and finite");
    }
    memcpy(c->light_dir, light_dir, sizeof(c->light_dir));
    memcpy(c->light_color, light_color, sizeof(c->light_color));
    memcpy(c->ambient, ambient, sizeof(c->ambient));
    return VXRT_OK;
}

int vxrt_set_fov(vxrt_ctx* c, float fov_degrees)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    c->fov = fov_degrees;
    return VXRT_OK;
}

int vxrt_set_ortho_window_size(vxrt_ctx* c, float sx, float sy)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    c->ortho[0] = sx;
    c->ortho[1] = sy;
    return VXRT_OK;
}

// GetDirections (Renderer.cu:27-42): float cos/sin, forward and up negated on return
void vxrt_get_directions(const float euler[3], float fwd[3], float up[3], float right[3])
{
    float fx = cosf(euler[0]) * sinf(euler[1]);
    float fy = -sinf(euler[0]);
    float fz = cosf(euler[0]) * cosf(euler[1]);
    float rx = cosf(euler[1]), ry = 0.0f, rz = -sinf(euler[1]);
    float ux = fy * rz - fz * ry, uy = fz * rx - fx * rz, uz = fx * ry - fy * rx;
    fwd[0] = fx * -1;
    fwd[1] = fy * -1;
    fwd[2] = fz * -1;
    up[0] = ux * -1;
    up[1] = uy * -1;
    up[2] = uz * -1;
    right[0] = rx;
    right[1] = ry;
    right[2] = rz;
}

void vxrt_render_flags_default(vxrt_render_flags* f)
{
    if (!f)
        return;
    memset(f, 0, sizeof(*f));
    f->struct_size = sizeof(*f);
    f->mode = VXRT_MODE_SHADED;
    f->frame_number = -1;
    f->strip_rows = 16;
    f->strip_count = 1;
    f->tile_schedule = 1;
}

uint32_t vxrt_compact_rows(uint32_t height, int32_t strip_rows, int32_t strip_count, int32_t strip_index)
{
    if (strip_rows <= 0 || strip_count <= 1)
        return height;
    uint32_t rows = 0;
    uint32_t nstrips = (height + (uint32_t)strip_rows - 1) / (uint32_t)strip_rows;
    for (uint32_t s = (uint32_t)strip_index; s < nstrips; s += (uint32_t)strip_count) {
        uint32_t begin = s * (uint32_t)strip_rows;
        uint32_t end = begin + (uint32_t)strip_rows < height ? begin + (uint32_t)strip_rows : height;
        rows += end - begin;
    }
    return rows;
}

// What camera_ray (vxrt_camera.hpp) reads of a launch besides the view: the frame size and getRayDirection's per-pixel
// constants (Renderer.cu:46,50-52), hoisted to the host.  One place for the render launches and vxrt_frame_guides, whose keys
// are defined by the renderer's own primary rays.
static void camera_args(const vxrt_ctx* c, uint32_t width, uint32_t height, vxrt::RenderArgs& A)
{
    A.width = width;
    A.height = height;
    float aspect = (float)width / (float)height;
    float fov = (float)((double)c->fov * 3.1415 / 180.0);
    A.kx = tanf(fov / 2.0f) * aspect;
    A.ky = tanf(fov / 2.0f);
    A.ratio = (float)width / (float)height;
    A.ortho_x = c->ortho[0];
    A.ortho_y = c->ortho[1];
    A.inv_width = 1.0f / (float)(int)width;
    A.inv_height = 1.0f / (float)(int)height;
}

// one launch for `nviews` views; nviews == 0: the single view `views[0]` through the single-view kernel arguments
static int render_launch(vxrt_ctx* c, uint32_t width, uint32_t height, unsigned nviews, const vxrt_view* views,
                         const vxrt_render_flags* fl)
{
    vxrt_render_flags def;
    if (!fl) {
        vxrt_render_flags_default(&def);
        fl = &def;
    }
    if (fl->struct_size != sizeof(vxrt_render_flags))
        return fail(VXRT_ERR_INVALID, "vxrt_render_flags size mismatch");
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    if (width == 0 || height == 0 || height > 65535u)
        return fail(VXRT_ERR_INVALID, "empty frame, or more than 65535 rows");
    if (fl->strip_count > 1 && (fl->strip_rows <= 0 || fl->strip_index < 0 || fl->strip_index >= fl->strip_count))
        return fail(VXRT_ERR_INVALID, "bad strip sharding");
    const unsigned n = nviews ? nviews : 1u;
    for (unsigned v = 0; v < n; ++v) {
        if (!views[v].d_fb)
            return fail(VXRT_ERR_INVALID, "a view has no framebuffer");
        // ray validity (include/vxrt.h): a camera with a non-finite component would hand every pixel an invalid ray
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(views[v].origin[a]) || !std::isfinite(views[v].fwd[a]) || !std::isfinite(views[v].up[a]) ||
                !std::isfinite(views[v].right[a]))
                return fail(VXRT_ERR_INVALID, "camera origin / forward / up / right must be finite numbers");
    }
    if (fl->d_accum && nviews != 0)
        return fail(VXRT_ERR_INVALID, "temporal accumulation (d_accum) is per view: use vxrt_render");
    if (fl->d_accum && (reinterpret_cast<uintptr_t>(fl->d_accum) & 15u))
        return fail(VXRT_ERR_INVALID, "d_accum must be 16-byte aligned");
    VX_HIP(hipSetDevice(c->device));
    hipStream_t stream = (hipStream_t)fl->stream;
    const bool capturing = vxrt::stream_capturing(stream);
    if (capturing) {  // (include/vxrt.h, "Stream capture": refused before anything is enqueued or counted)
        for (unsigned v = 0; v < n; ++v)
            if (views[v].frame_number < 0)
                return fail(VXRT_ERR_INVALID, "stream capture: frame_number < 0 would bake the context's frame counter into the graph; pass an explicit frame_number");
        if (nviews != 0 && c->kernel_variant != 1 && !c->d_views)
            return fail(VXRT_ERR_INVALID, "stream capture: the context's view slots are allocated by its first multi-view launch; issue one vxrt_render_views launch before capturing");
    }

    vxrt::RenderArgs A;
    memset(&A, 0, sizeof(A));
    A.W = c->view;
    camera_args(c, width, height, A);
    A.light_dir = vxrt::f3{c->light_dir[0], c->light_dir[1], c->light_dir[2]};
    {   // unit3() of vxrt_device.hpp on the host: v * (1 / sqrt(dot(v, v))), binary32 throughout, no contraction
        const float lx = c->light_dir[0], ly = c->light_dir[1], lz = c->light_dir[2];
        const float dd = lx * lx + ly * ly + lz * lz;
        const float inv = 1.0f / sqrtf(dd);
        A.light_unit = vxrt::f3{lx * inv, ly * inv, lz * inv};
        A.light_step = vxrt::f3{A.light_unit.x * 0.01f, A.light_unit.y * 0.01f, A.light_unit.z * 0.01f};
    }
    A.light_color = vxrt::f3{c->light_color[0], c->light_color[1], c->light_color[2]};
    A.ambient = vxrt::f3{c->ambient[0], c->ambient[1], c->ambient[2]};
    A.mode = fl->mode;
    A.checkerboard = fl->checkerboard ? 1 : 0;
    A.shadow = fl->shadow ? 1 : 0;
    A.bounce_samples = fl->bounce_samples < 0 ? 0 : fl->bounce_samples;
    A.bounce_samples_f = (float)A.bounce_samples;
    A.inv_bounce_samples = A.bounce_samples > 0 ? 1.0f / A.bounce_samples_f : 0.0f;
    A.bounce_all_hits = fl->bounce_all_hits ? 1 : 0;
    A.bounce_depth = fl->bounce_depth >= 2 ? 2 : 1;
    A.ortho = fl->ortho ? 1 : 0;
    A.strip_rows = fl->strip_rows > 0 ? fl->strip_rows : 16;
    A.strip_count = fl->strip_count > 1 ? fl->strip_count : 1;
    A.strip_index = fl->strip_index;
    A.compact = fl->compact ? 1 : 0;
    A.accum = reinterpret_cast<float4*>(fl->d_accum);
    A.accum_reset = fl->accum_reset ? 1 : 0;
    A.strip_shift = -1;
    for (int b = 0; b < 31; ++b)
        if (A.strip_rows == (1 << b))
            A.strip_shift = b;
    // launch shape: RenderScreen halves the rows under checkerboard (Renderer.cu:311-316); a shard
    // without checkerboard launches only its own rows
    if (A.checkerboard)
        A.launch_rows = height >> 1;
    else if (A.strip_count > 1)
        A.launch_rows = vxrt_compact_rows(height, A.strip_rows, A.strip_count, A.strip_index);
    else
        A.launch_rows = height;
    A.stats = c->d_stats;  // counters accumulate until vxrt_frame_stats_get reads and clears them
    A.persistent_waves = c->persistent_waves;
    const bool persistent = c->kernel_variant != 1;
    const bool schedule = fl->tile_schedule && persistent;

    auto frame_number_of = [&](const vxrt_view& v) -> uint32_t {
        if (v.frame_number >= 0)
            return (uint32_t)v.frame_number;
        return c->frame_counter++;  // the copy precedes the increment, Renderer.cu:310,322
    };
    auto f3_of = [](const float* p) { return vxrt::f3{p[0], p[1], p[2]}; };

    if (nviews == 0 || !persistent) {  // single-view kernel arguments; variant 1 takes the views one by one
        for (unsigned v = 0; v < n; ++v) {
            A.frame_number = frame_number_of(views[v]);
            A.origin = f3_of(views[v].origin);
            A.fwd = f3_of(views[v].fwd);
            A.up = f3_of(views[v].up);
            A.right = f3_of(views[v].right);
            A.fb = (uint8_t*)views[v].d_fb;
            A.color_aov = views[v].d_color_aov;
            A.hit_aov = (long long*)views[v].d_hit_aov;
            A.want_hit_aov = A.hit_aov != nullptr;
            A.tile_order = nviews == 0 ? fl->d_tile_order : nullptr;
            A.row_order_n = 0;
            if (schedule && !A.tile_order)
                vxrt::schedule_tile_rows(A, A.fwd, A.up, A.row_order, A.row_order_n);
            const unsigned slot = c->launch_seq.fetch_add(1u) % kTileCounterRing;
            VX_HIP(vxrt::ring_acquire(c->counter_busy[slot], capturing));
            A.tile_counter = c->d_queues + (size_t)slot * vxrt::kQueueWords;
            VX_HIP(vxrt::launch_render(A, fl->collect_stats != 0, c->kernel_variant, stream));
            VX_HIP(hipGetLastError());
            VX_HIP(vxrt::ring_release(c->counter_busy[slot], stream, capturing));
        }
        return VXRT_OK;
    }

    // multi-view launch: the per-view arguments travel through a ring of device slots (stream-ordered copy)
    if (!c->d_views)
        VX_HIP(hipMalloc((void**)&c->d_views, sizeof(vxrt::ViewArgs) * vxrt::kMaxViews * kViewSlots));
    std::vector<vxrt::ViewArgs> host(n);
    for (unsigned v = 0; v < n; ++v) {
        vxrt::ViewArgs& S = host[v];
        memset(&S, 0, sizeof(S));
        S.origin = f3_of(views[v].origin);
        S.fwd = f3_of(views[v].fwd);
        S.up = f3_of(views[v].up);
        S.right = f3_of(views[v].right);
        S.frame_number = frame_number_of(views[v]);
        S.fb = (uint8_t*)views[v].d_fb;
        S.color_aov = views[v].d_color_aov;
        S.hit_aov = (long long*)views[v].d_hit_aov;
        A.want_hit_aov |= S.hit_aov != nullptr;
        if (schedule)
            vxrt::schedule_tile_rows(A, S.fwd, S.up, S.row_order, S.row_order_n);
    }
    const unsigned vslot = c->view_seq.fetch_add(1u) % kViewSlots, cslot = c->launch_seq.fetch_add(1u) % kTileCounterRing;
    VX_HIP(vxrt::ring_acquire(c->views_busy[vslot], capturing));
    VX_HIP(vxrt::ring_acquire(c->counter_busy[cslot], capturing));
    vxrt::ViewArgs* slot = c->d_views + (size_t)vslot * vxrt::kMaxViews;
    if (!capturing) {
        VX_HIP(hipMemcpyAsync(slot, host.data(), sizeof(vxrt::ViewArgs) * n, hipMemcpyHostToDevice, stream));
    } else {  // a graph owns what its replays read: the views travel as kernel arguments, not through `host`
        for (unsigned v = 0; v < n; ++v)
            hipLaunchKernelGGL(vxrt::k_store_view, dim3(1), dim3(64), 0, stream, host[v], slot + v);
        VX_HIP(hipGetLastError());
    }
    A.views = slot;
    A.nviews = n;
    A.tile_counter = c->d_queues + (size_t)cslot * vxrt::kQueueWords;
    VX_HIP(vxrt::launch_render(A, fl->collect_stats != 0, c->kernel_variant, stream));
    VX_HIP(hipGetLastError());
    VX_HIP(vxrt::ring_release(c->views_busy[vslot], stream, capturing));
    VX_HIP(vxrt::ring_release(c->counter_busy[cslot], stream, capturing));
    return VXRT_OK;
}

int vxrt_render(vxrt_ctx* c, uint32_t width, uint32_t height, void* d_fb, const float origin[3], const float fwd[3],
                const float up[3], const float right[3], const vxrt_render_flags* fl)
{
    if (!c || !d_fb || !origin || !fwd || !up || !right)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    vxrt_view v;
    memset(&v, 0, sizeof(v));
    v.d_fb = d_fb;
    for (int a = 0; a < 3; ++a) {
        v.origin[a] = origin[a];
        v.fwd[a] = fwd[a];
        v.up[a] = up[a];
        v.right[a] = right[a];
    }
    v.frame_number = fl ? fl->frame_number : -1;
    v.d_color_aov = fl ? fl->d_color_aov : nullptr;
    v.d_hit_aov = fl ? fl->d_hit_aov : nullptr;
    return render_launch(c, width, height, 0, &v, fl);
}

int vxrt_render_views(vxrt_ctx* c, uint32_t width, uint32_t height, uint32_t n_views, const vxrt_view* views,
                      const vxrt_render_flags* fl)
{
    if (!c || !views)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (n_views == 0 || n_views > vxrt::kMaxViews)
        return fail(VXRT_ERR_INVALID, "between 1 and 16 views per launch");
    return render_launch(c, width, height, n_views, views, fl);
}

int vxrt_frame_stats_get(vxrt_ctx* c, vxrt_frame_stats* out)
{
    if (!c || !out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());  // every stream of the device, non-blocking ones included
    unsigned long long now[vxrt::kStatCount] = {}, h[vxrt::kStatCount];
    std::vector<unsigned long long> rows((size_t)vxrt::kStatRows * vxrt::kStatRowStride);
    VX_HIP(hipMemcpy(rows.data(), c->d_stats, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (unsigned r = 0; r < vxrt::kStatRows; ++r)
        for (int i = 0; i < vxrt::kStatCount; ++i)
            now[i] += rows[(size_t)r * vxrt::kStatRowStride + i];
    for (int i = 0; i < vxrt::kStatCount; ++i) {  // what was added since the previous read; the device copy only grows
        h[i] = now[i] - c->stats_base[i];
        c->stats_base[i] = now[i];
    }
    out->primary_rays = h[vxrt::kStatPrimary];
    out->shadow_rays = h[vxrt::kStatShadow];
    out->bounce_rays = h[vxrt::kStatBounce];
    out->primary_hits = h[vxrt::kStatPrimaryHits];
    out->coarse_probes = h[vxrt::kStatCoarseProbes];
    out->brick_entries = h[vxrt::kStatBrickEntries];
    out->fine_probes = h[vxrt::kStatFineProbes];
    out->dbg[0] = h[vxrt::kStatDbgIters];
    out->dbg[1] = h[vxrt::kStatDbgWalkLanes];
    out->dbg[2] = h[vxrt::kStatDbgEndRuns];
    out->dbg[3] = h[vxrt::kStatDbgBoxRuns];
    out->dbg[4] = h[vxrt::kStatDbgNextRuns];
    out->dbg[5] = h[vxrt::kStatDbgEndLanes];
    out->dbg[6] = h[vxrt::kStatDbgBoxLanes];
    out->dbg[7] = h[vxrt::kStatDbgNextLanes];
    out->dbg[8] = h[vxrt::kStatDbgLifetime];
    out->dbg[9] = h[vxrt::kStatDbgDrained];
    out->dbg[10] = h[vxrt::kStatDbgNextTicks];
    out->dbg[11] = h[vxrt::kStatDbgParkTicks];
    out->dbg[12] = h[vxrt::kStatDbgEndShadow];
    out->guard_slack_loads = h[vxrt::kStatGuardSlack];
    out->guard_stray_loads = h[vxrt::kStatGuardStray];
#ifdef VXRT_EXPERIMENTS  // (vxrt_frame_stats has no field for them: a development print of the A/B build)
    if (getenv("VXRT_PRINT_COSTART"))
        fprintf(stderr, "vxrt: rounds with the end-of-walk and the ray-finished phase %llu, with walk starts from both %llu, of %llu rounds\n",
                h[vxrt::kStatDbgCoRuns], h[vxrt::kStatDbgCoStarts], h[vxrt::kStatDbgIters]);
#endif
    return VXRT_OK;
}

int vxrt_deinterleave_strips(vxrt_ctx* c, uint32_t width, uint32_t height, int32_t strip_rows, int32_t strip_count,
                             const void* d_shards, uint64_t shard_stride_bytes, void* d_fb, void* stream)
{
    if (!c || !d_shards || !d_fb)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (width % 4 != 0 || shard_stride_bytes % 16 != 0 || strip_rows <= 0 || strip_count <= 0)
        return fail(VXRT_ERR_INVALID, "width must be a multiple of 4 pixels and the shard stride of 16 bytes");
    VX_HIP(hipSetDevice(c->device));
    vxrt::launch_deinterleave(d_shards, shard_stride_bytes, d_fb, width, height, (uint32_t)strip_rows,
                              (uint32_t)strip_count, (hipStream_t)stream);
    VX_HIP(hipGetLastError());
    return VXRT_OK;
}

int vxrt_deinterleave_views(vxrt_ctx* c, uint32_t width, uint32_t height, int32_t strip_rows, int32_t strip_count,
                            const void* d_shards, uint64_t shard_stride_bytes, uint64_t view_stride_bytes, uint32_t n_views,
                            void* d_fb, uint64_t fb_stride_bytes, void* stream)
{
    if (!c || !d_shards || !d_fb)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (width % 4 != 0 || shard_stride_bytes % 16 != 0 || view_stride_bytes % 16 != 0 || fb_stride_bytes % 16 != 0 ||
        strip_rows <= 0 || strip_count <= 0)
        return fail(VXRT_ERR_INVALID, "width must be a multiple of 4 pixels and the strides of 16 bytes");
    if (n_views > 65535u)
        return fail(VXRT_ERR_INVALID, "too many views");
    VX_HIP(hipSetDevice(c->device));
    vxrt::launch_deinterleave(d_shards, shard_stride_bytes, d_fb, width, height, (uint32_t)strip_rows, (uint32_t)strip_count,
                              (hipStream_t)stream, n_views, view_stride_bytes, fb_stride_bytes);
    VX_HIP(hipGetLastError());
    return VXRT_OK;
}

int vxrt_trace_batch(vxrt_ctx* c, const float* d_origins, const float* d_dirs, uint64_t n, float* d_pos,
                     float* d_normal, int32_t* d_steps, uint8_t* d_hit, int64_t* d_voxel, vxrt_frame_stats* stats,
                     void* stream_)
{
    if (!c || (n && (!d_origins || !d_dirs || !d_pos || !d_normal || !d_steps)))
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    VX_HIP(hipSetDevice(c->device));
    hipStream_t stream = (hipStream_t)stream_;
    const bool capturing = vxrt::stream_capturing(stream);
    if (capturing && stats)  // (include/vxrt.h, "Stream capture": refused before anything is enqueued or counted)
        return fail(VXRT_ERR_INVALID, "stream capture: a batch with stats synchronises with the host; pass stats_or_null = NULL and read vxrt_frame_stats_get after the replays");
    vxrt::BatchArgs B;
    memset(&B, 0, sizeof(B));
    B.W = c->view;
    B.origins = d_origins;
    B.dirs = d_dirs;
    B.n = n;
    B.pos = d_pos;
    B.normal = d_normal;
    B.steps = d_steps;
    B.hit = d_hit;
    B.voxel = (long long*)d_voxel;
    B.stats = c->d_stats;
    const unsigned tslot = c->launch_seq.fetch_add(1u) % kTileCounterRing;
    VX_HIP(vxrt::ring_acquire(c->counter_busy[tslot], capturing));
    B.ticket = c->d_queues + (size_t)tslot * vxrt::kQueueWords;
    B.persistent_waves = c->persistent_waves;
    B.max_steps = c->batch_max_steps;
    if (stats) {  // a stats request reports what ran between two device-wide syncs: this batch alone if nothing else is submitted
        vxrt_frame_stats drop;
        int rc = vxrt_frame_stats_get(c, &drop);
        if (rc)
            return rc;
    }
    VX_HIP(vxrt::launch_trace_batch(B, stats != nullptr, c->kernel_variant, stream));
    VX_HIP(hipGetLastError());
    VX_HIP(vxrt::ring_release(c->counter_busy[tslot], stream, capturing));
    if (stats) {
        VX_HIP(hipStreamSynchronize(stream));
        return vxrt_frame_stats_get(c, stats);
    }
    return VXRT_OK;
}

int vxrt_set_batch_max_steps(vxrt_ctx* c, int32_t max_steps)
{
    if (!c || max_steps < 1 || max_steps > vxrt::kMaxSteps)
        return fail(VXRT_ERR_INVALID, "max_steps must be in [1, 2048]");
    c->batch_max_steps = max_steps;
    return VXRT_OK;
}

int vxrt_trace_batch_host(vxrt_ctx* c, const float* origins, const float* dirs, uint64_t n, float* pos, float* normal,
                          int32_t* steps, uint8_t* hit, int64_t* voxel, vxrt_frame_stats* stats)
{
    if (!c || (n && (!origins || !dirs || !pos || !normal || !steps)))
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    if (n == 0)
        return VXRT_OK;
    VX_HIP(hipSetDevice(c->device));
    float *d_o = nullptr, *d_d = nullptr, *d_p = nullptr, *d_n = nullptr;
    int32_t* d_s = nullptr;
    uint8_t* d_h = nullptr;
    int64_t* d_v = nullptr;
    int rc = VXRT_OK;
    auto cleanup = [&]() {
        (void)hipFree(d_o); (void)hipFree(d_d); (void)hipFree(d_p); (void)hipFree(d_n);
        (void)hipFree(d_s); (void)hipFree(d_h); (void)hipFree(d_v);
    };
#define VX_TRY(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            cleanup();                                                                     \
            return fail(VXRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));  \
        }                                                                                  \
    } while (0)
    VX_TRY(hipMalloc((void**)&d_o, n * 12));
    VX_TRY(hipMalloc((void**)&d_d, n * 12));
    VX_TRY(hipMalloc((void**)&d_p, n * 12));
    VX_TRY(hipMalloc((void**)&d_n, n * 12));
    VX_TRY(hipMalloc((void**)&d_s, n * 4));
    VX_TRY(hipMalloc((void**)&d_h, n));
    VX_TRY(hipMalloc((void**)&d_v, n * 8));
    VX_TRY(hipMemcpy(d_o, origins, n * 12, hipMemcpyHostToDevice));
    VX_TRY(hipMemcpy(d_d, dirs, n * 12, hipMemcpyHostToDevice));
    rc = vxrt_trace_batch(c, d_o, d_d, n, d_p, d_n, d_s, d_h, d_v, stats, nullptr);
    if (rc == VXRT_OK) {
        VX_TRY(hipDeviceSynchronize());
        VX_TRY(hipMemcpy(pos, d_p, n * 12, hipMemcpyDeviceToHost));
        VX_TRY(hipMemcpy(normal, d_n, n * 12, hipMemcpyDeviceToHost));
        VX_TRY(hipMemcpy(steps, d_s, n * 4, hipMemcpyDeviceToHost));
        if (hit) VX_TRY(hipMemcpy(hit, d_h, n, hipMemcpyDeviceToHost));
        if (voxel) VX_TRY(hipMemcpy(voxel, d_v, n * 8, hipMemcpyDeviceToHost));
    }
#undef VX_TRY
    cleanup();
    return rc;
}

// ---- brickmap file: the resident tables as they lie in HBM, behind a versioned header ------
namespace {

constexpr char kFileMagic[8] = {'V', 'X', 'B', 'R', 'K', 'M', 'A', 'P'};
constexpr uint32_t kFileVersion = 2;  // 2: position-sensitive stream checksums (sum + sum of running sums)
constexpr size_t kFileChunk = 64u << 20;  // staging buffer for the table streams

struct FileHeader {  // 120 bytes, little endian
    char magic[8];
    uint32_t version, header_bytes;
    int32_t factor, cdims[3];
    uint64_t ncells, nslots;
    uint64_t coarse_bytes, meta_bytes, pool_bytes;  // the three table streams, in this order after the header
    uint64_t sum[3];                                 // per stream: a = sum of its 32-bit words, mod 2^64
    uint64_t sum2[3];                                // per stream: b = sum of the running values of a (Fletcher style):
                                                     // unlike a alone, it changes when words are swapped or moved
};
static_assert(sizeof(FileHeader) == 120, "file header layout");

struct StreamSum {
    uint64_t a = 0, b = 0;
    void add(const void* p, size_t bytes)
    {
        const uint32_t* w = static_cast<const uint32_t*>(p);
        uint64_t a_ = a, b_ = b;
        for (size_t i = 0; i < bytes / 4; ++i) {
            a_ += w[i];
            b_ += a_;
        }
        a = a_;
        b = b_;
    }
};

struct FileCloser {
    FILE* f;
    ~FileCloser() { if (f) fclose(f); }
};

int read_header(FILE* f, const char* path, FileHeader& h)
{
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, kFileMagic, 8) != 0)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": not a brickmap file");
    if (h.version != kFileVersion || h.header_bytes != sizeof(FileHeader))
        return fail(VXRT_ERR_INVALID, std::string(path) + ": unsupported brickmap file version");
    int cd[3] = {h.cdims[0], h.cdims[1], h.cdims[2]};
    int rc = vxrt::check_shape(h.factor, cd);
    if (rc)
        return rc;
    const uint64_t ncells = (uint64_t)cd[0] * cd[1] * cd[2], bw = (uint64_t)h.factor * h.factor * h.factor / 32;
    if (h.ncells != ncells || h.nslots > ncells || h.coarse_bytes != ((ncells + 31) / 32) * 4 ||
        h.meta_bytes != ncells * sizeof(uint2) || h.pool_bytes != h.nslots * bw * 4)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": header sizes are inconsistent");
    return VXRT_OK;
}

}  // namespace

int vxrt_world_file_info(const char* path, vxrt_world_info* out)
{
    if (!path || !out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": cannot open");
    FileHeader h;
    int rc = read_header(fc.f, path, h);
    if (rc)
        return rc;
    out->factor = h.factor;
    for (int a = 0; a < 3; ++a)
        out->cdims[a] = h.cdims[a];
    out->ncells = h.ncells;
    out->nslots = h.nslots;
    out->hbm_bytes = h.coarse_bytes + h.meta_bytes + h.pool_bytes;
    return VXRT_OK;
}

int vxrt_save_world(vxrt_ctx* c, const char* path)
{
    if (!c || !path)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());
    FileHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kFileMagic, 8);
    h.version = kFileVersion;
    h.header_bytes = sizeof(FileHeader);
    h.factor = c->view.f;
    h.cdims[0] = c->view.cx;
    h.cdims[1] = c->view.cy;
    h.cdims[2] = c->view.cz;
    h.ncells = c->ncells;
    h.nslots = c->nslots;
    h.coarse_bytes = ((c->ncells + 31) / 32) * 4;
    h.meta_bytes = c->ncells * sizeof(uint2);
    h.pool_bytes = c->nslots * (uint64_t)c->view.brick_words * 4;
    FileCloser fc{fopen(path, "wb")};
    if (!fc.f)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": cannot create");
    if (fwrite(&h, sizeof(h), 1, fc.f) != 1)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": write failed");
    // the file holds the tables in the reference's tiled order: re-ordered on the device, then streamed out (the two
    // cell tables through whole-table temporaries, the pool through a staging buffer of kFileChunk bytes)
    std::vector<unsigned char> stage(kFileChunk);
    const int cd[3] = {c->view.cx, c->view.cy, c->view.cz};
    struct Temps {
        uint32_t *coarse = nullptr, *pool = nullptr, *order = nullptr;
        uint2* meta = nullptr;
        ~Temps() { (void)hipFree(coarse); (void)hipFree(meta); (void)hipFree(pool); (void)hipFree(order); }
    } T;
    VX_HIP(hipMalloc((void**)&T.coarse, h.coarse_bytes));
    VX_HIP(hipMalloc((void**)&T.meta, h.meta_bytes));
    VX_HIP(vxrt::layout_bits(c->d_coarse, T.coarse, cd, false));
    VX_HIP(vxrt::layout_meta(c->d_meta, T.meta, cd, false));
    // A world changed by vxrt_edit_voxels holds freed slots and bricks out of cell order: the file gets its live bricks
    // only, renumbered in the tiled cell order of the tables (as the builders number them), gathered by new number.
    std::vector<uint32_t> order;  // old slot of every brick of the file
    if (c->edited) {
        std::vector<uint2> meta(c->ncells);
        VX_HIP(hipMemcpy(meta.data(), T.meta, h.meta_bytes, hipMemcpyDeviceToHost));
        for (uint2& m : meta)
            if (m.x != VXRT_EMPTY_SLOT) {
                order.push_back(m.x);
                m.x = (uint32_t)(order.size() - 1);
            }
        VX_HIP(hipMemcpy(T.meta, meta.data(), h.meta_bytes, hipMemcpyHostToDevice));
        h.nslots = order.size();
        h.pool_bytes = h.nslots * (uint64_t)c->view.brick_words * 4;
        VX_HIP(hipMalloc((void**)&T.order, std::max<size_t>(4, order.size() * sizeof(uint32_t))));
        if (!order.empty())
            VX_HIP(hipMemcpy(T.order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    VX_HIP(hipMalloc((void**)&T.pool, std::max<uint64_t>(4, std::min<uint64_t>(kFileChunk, h.pool_bytes))));
    const void* src[3] = {T.coarse, T.meta, nullptr};
    const uint64_t bytes[3] = {h.coarse_bytes, h.meta_bytes, h.pool_bytes};
    const uint64_t brick_bytes = (uint64_t)c->view.brick_words * 4;
    for (int t = 0; t < 3; ++t) {
        StreamSum cs;
        for (uint64_t off = 0; off < bytes[t]; off += kFileChunk) {
            const size_t n = (size_t)std::min<uint64_t>(kFileChunk, bytes[t] - off);
            if (t == 2 && c->edited) {  // compacted: gather by new number, then re-order in place
                VX_HIP(vxrt::gather_bricks(c->d_pool, T.order + off / brick_bytes, (uint32_t)(n / brick_bytes), T.pool, c->view.f));
                VX_HIP(vxrt::layout_bricks(T.pool, T.pool, n / brick_bytes, c->view.f, false));
                VX_HIP(hipMemcpy(stage.data(), T.pool, n, hipMemcpyDeviceToHost));
            } else if (t == 2) {  // kFileChunk is a whole number of bricks
                VX_HIP(vxrt::layout_bricks(c->d_pool + off / 4, T.pool, n / brick_bytes, c->view.f, false));
                VX_HIP(hipMemcpy(stage.data(), T.pool, n, hipMemcpyDeviceToHost));
            } else {
                VX_HIP(hipMemcpy(stage.data(), static_cast<const unsigned char*>(src[t]) + off, n, hipMemcpyDeviceToHost));
            }
            cs.add(stage.data(), n);
            if (fwrite(stage.data(), 1, n, fc.f) != n)
                return fail(VXRT_ERR_INVALID, std::string(path) + ": write failed (disk full?)");
        }
        h.sum[t] = cs.a;
        h.sum2[t] = cs.b;
    }
    if (fseek(fc.f, 0, SEEK_SET) != 0 || fwrite(&h, sizeof(h), 1, fc.f) != 1 || fflush(fc.f) != 0)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": write failed");
    return VXRT_OK;
}

int vxrt_load_world(vxrt_ctx* c, const char* path)
{
    if (!c || !path)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": cannot open");
    FileHeader h;
    int rc = read_header(fc.f, path, h);
    if (rc)
        return rc;
    VX_HIP(hipSetDevice(c->device));
    int cd[3] = {h.cdims[0], h.cdims[1], h.cdims[2]};
    rc = vxrt::alloc_world(c, h.factor, cd, h.nslots);
    if (rc)
        return rc;
    // stream the tables into HBM, checking on the way what vxrt_upload_world checks: every occupied coarse cell
    // owns a brick inside the pool, every empty one owns none
    std::vector<unsigned char> stage(kFileChunk);
    std::vector<uint32_t> coarse(h.coarse_bytes / 4);
    // the file's tables are in the reference's tiled order: the two cell tables land in device temporaries and are
    // re-ordered into the HBM order when their stream is complete, the pool piece by piece in place
    struct Temps {
        uint32_t* coarse = nullptr;
        uint2* meta = nullptr;
        ~Temps() { (void)hipFree(coarse); (void)hipFree(meta); }
    } T;
    auto bad = [&](const std::string& why) {
        vxrt::free_world(c);
        return fail(VXRT_ERR_INVALID, std::string(path) + ": " + why);
    };
    auto bad_hip = [&](hipError_t e) {
        vxrt::free_world(c);
        return fail(VXRT_ERR_HIP, std::string("world load: ") + hipGetErrorString(e));
    };
    hipError_t e = hipMalloc((void**)&T.coarse, h.coarse_bytes);
    if (e == hipSuccess)
        e = hipMalloc((void**)&T.meta, h.meta_bytes);
    if (e != hipSuccess)
        return bad_hip(e);
    void* dst[3] = {T.coarse, T.meta, c->d_pool};
    const uint64_t bytes[3] = {h.coarse_bytes, h.meta_bytes, h.pool_bytes};
    const uint64_t brick_bytes = (uint64_t)h.factor * h.factor * h.factor / 8;
    for (int t = 0; t < 3; ++t) {
        StreamSum cs;
        for (uint64_t off = 0; off < bytes[t]; off += kFileChunk) {
            const size_t n = (size_t)std::min<uint64_t>(kFileChunk, bytes[t] - off);
            if (fread(stage.data(), 1, n, fc.f) != n)
                return bad("file is truncated");
            cs.add(stage.data(), n);
            if (t == 0)
                memcpy(reinterpret_cast<unsigned char*>(coarse.data()) + off, stage.data(), n);
            if (t == 1) {
                const uint2* m = reinterpret_cast<const uint2*>(stage.data());
                const uint64_t first = off / sizeof(uint2);
                for (size_t i = 0; i < n / sizeof(uint2); ++i) {
                    const uint64_t cell = first + i;
                    const bool bit = (coarse[cell >> 5] >> (cell & 31)) & 1u;
                    if (bit ? m[i].x >= h.nslots : m[i].x != VXRT_EMPTY_SLOT)
                        return bad("cell table does not match the coarse bits / pool size");
                    if (bit && !vxrt::extents_valid(m[i].y, h.factor))
                        return bad("brick extents outside the brick");
                }
            }
            e = hipMemcpy(static_cast<unsigned char*>(dst[t]) + off, stage.data(), n, hipMemcpyHostToDevice);
            if (e == hipSuccess && t == 2)  // kFileChunk is a whole number of bricks
                e = vxrt::layout_bricks(c->d_pool + off / 4, c->d_pool + off / 4, n / brick_bytes, h.factor, true);
            if (e != hipSuccess)
                return bad_hip(e);
        }
        if (cs.a != h.sum[t] || cs.b != h.sum2[t])
            return bad("checksum mismatch (corrupt file)");
        if (t == 0)
            e = vxrt::layout_bits(T.coarse, c->d_coarse, cd, true);
        if (t == 1)
            e = vxrt::layout_meta(T.meta, c->d_meta, cd, true);
        if (e != hipSuccess)
            return bad_hip(e);
    }
    e = hipDeviceSynchronize();
    if (e != hipSuccess)
        return bad_hip(e);
    c->nslots = h.nslots;
    vxrt::fill_view(c, h.factor, cd);
    c->has_world = true;
    return VXRT_OK;
}

}  // extern "C"

// ---- chunk streaming (include/vxrt.h): coarse tables of the whole world resident, brick data only near the focus --------
// The bookkeeping -- chunk table, order, radius test, eviction scan, pool allocator -- is vxrt::StreamPolicy
// (vxrt_stream.hpp, host only); this file adds the file, the device tables and the pool.
struct StreamState {
    FILE* f = nullptr;
    FileHeader h{};
    uint64_t pool_off = 0, brick_bytes = 0;
    std::vector<uint32_t> coarse;             // the whole world's coarse bits
    std::vector<vxrt::StreamCell> meta;       // ... and cell records, with the FILE's slot numbers
    vxrt::StreamPolicy P;
    uint2* d_chunk_meta = nullptr;            // device staging for one chunk's 512 cell records
};
static_assert(sizeof(vxrt::StreamCell) == sizeof(uint2), "a cell record is 8 bytes in the file and on the device");

namespace {
// the loads and evictions of vxrt_stream_focus: file reads, copies into the pool and the two re-ordering launches
struct StreamDeviceIO final : vxrt::StreamIO {
    vxrt_ctx* c;
    StreamState* S;
    std::vector<unsigned char> stage;
    std::vector<uint2> meta = std::vector<uint2>(512);
    StreamDeviceIO(vxrt_ctx* c_, StreamState* S_) : c(c_), S(S_) {}

    int load(uint32_t, uint32_t first_slot, uint32_t nbricks, uint64_t start) override
    {
        const uint64_t nbytes = (uint64_t)nbricks * S->brick_bytes;
        stage.resize(nbytes);
        if (fseek(S->f, (long)(S->pool_off + (uint64_t)first_slot * S->brick_bytes), SEEK_SET) != 0 ||
            fread(stage.data(), 1, nbytes, S->f) != nbytes)
            return fail(VXRT_ERR_INVALID, "brickmap file: chunk read failed");
        hipError_t e = hipMemcpy(reinterpret_cast<unsigned char*>(c->d_pool) + start * S->brick_bytes, stage.data(), nbytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) {  // the file's bricks are in the reference's tiled bit order: into the HBM order, in place
            uint32_t* at = c->d_pool + start * (S->brick_bytes / 4);
            e = vxrt::layout_bricks(at, at, nbricks, S->h.factor, true);
        }
        if (e != hipSuccess)
            return fail(VXRT_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
        return VXRT_OK;
    }

    int tables(uint32_t ch, bool resident, int64_t base) override
    {
        uint32_t k = 0;
        for (uint64_t i = 0; i < 512; ++i) {
            const vxrt::StreamCell m = S->meta[(uint64_t)ch * 512 + i];
            meta[i] = (resident && m.slot != VXRT_EMPTY_SLOT) ? make_uint2((uint32_t)(base + k++), m.extents) : make_uint2(VXRT_EMPTY_SLOT, 0u);
        }
        // the chunk's 512 records (file order: the reference's tiled order, one chunk = one tile) go to their places in
        // the HBM tables -- 64 rows of 8 cells -- with their coarse bits
        VX_HIP(hipMemcpy(S->d_chunk_meta, meta.data(), 512 * sizeof(uint2), hipMemcpyHostToDevice));
        const int tw = S->h.cdims[0] / 8, th = S->h.cdims[1] / 8;
        VX_HIP(vxrt::chunk_tables(c->d_meta, c->d_coarse, S->d_chunk_meta, (int)(ch % (uint32_t)tw), (int)((ch / (uint32_t)tw) % (uint32_t)th),
                                  (int)(ch / ((uint32_t)tw * (uint32_t)th)), S->h.cdims[0], S->h.cdims[2]));
        return VXRT_OK;
    }
};
}  // namespace

namespace vxrt {
void stream_drop(vxrt_ctx* c)
{
    if (!c->stream)
        return;
    if (c->stream->f)
        fclose(c->stream->f);
    (void)hipFree(c->stream->d_chunk_meta);
    delete c->stream;
    c->stream = nullptr;
}
}  // namespace vxrt

extern "C" {

int vxrt_stream_open(vxrt_ctx* c, const char* path, uint64_t pool_capacity_bricks)
{
    if (!c || !path || pool_capacity_bricks == 0)
        return fail(VXRT_ERR_INVALID, "NULL argument or empty pool");
    if (pool_capacity_bricks > (uint64_t)VXRT_EMPTY_SLOT)  // slot numbers are 32 bits, and VXRT_EMPTY_SLOT is none
        return fail(VXRT_ERR_INVALID, "pool capacity above 0xFFFFFFFF bricks");
    FILE* f = fopen(path, "rb");
    if (!f)
        return fail(VXRT_ERR_INVALID, std::string(path) + ": cannot open");
    StreamState* S = new (std::nothrow) StreamState();
    if (!S) {
        fclose(f);
        return fail(VXRT_ERR_NOMEM, "out of host memory");
    }
    S->f = f;
    auto bad = [&](int code, const std::string& why) {
        fclose(S->f);
        delete S;
        return fail(code, why);
    };
    int rc = read_header(f, path, S->h);
    if (rc) {
        fclose(S->f);
        delete S;
        return rc;
    }
    const FileHeader& h = S->h;
    S->coarse.resize(h.coarse_bytes / 4);
    S->meta.resize(h.ncells);
    if (fread(S->coarse.data(), 1, h.coarse_bytes, f) != h.coarse_bytes || fread(S->meta.data(), 1, h.meta_bytes, f) != h.meta_bytes)
        return bad(VXRT_ERR_INVALID, std::string(path) + ": file is truncated");
    {   // the two table streams are checked like vxrt_load_world checks them (the pool is read chunk by chunk later)
        StreamSum a, b;
        a.add(S->coarse.data(), h.coarse_bytes);
        b.add(S->meta.data(), h.meta_bytes);
        if (a.a != h.sum[0] || a.b != h.sum2[0] || b.a != h.sum[1] || b.b != h.sum2[1])
            return bad(VXRT_ERR_INVALID, std::string(path) + ": checksum mismatch (corrupt file)");
    }
    S->pool_off = sizeof(FileHeader) + h.coarse_bytes + h.meta_bytes;
    S->brick_bytes = (uint64_t)h.factor * h.factor * h.factor / 8;
    int cd[3] = {h.cdims[0], h.cdims[1], h.cdims[2]};
    if (const char* why = S->P.init(h.factor, cd, S->coarse.data(), S->meta.data(), h.nslots, pool_capacity_bricks))
        return bad(VXRT_ERR_INVALID, std::string(path) + ": " + why);
    // device: the whole world's tables (all empty for now) + a pool of the requested capacity
    if (hipSetDevice(c->device) != hipSuccess)
        return bad(VXRT_ERR_HIP, "hipSetDevice");
    (void)hipDeviceSynchronize();
    rc = vxrt::alloc_world(c, h.factor, cd, pool_capacity_bricks);  // (frees a previous world, streamed or not)
    if (rc) {
        fclose(S->f);
        delete S;
        return rc;
    }
    std::vector<uint2> empty(h.ncells, make_uint2(VXRT_EMPTY_SLOT, 0u));
    hipError_t e = hipMemset(c->d_coarse, 0, h.coarse_bytes);
    if (e == hipSuccess)  // the cache pool starts as empty space, not as whatever the allocation held
        e = hipMemset(c->d_pool, 0, pool_capacity_bricks * S->brick_bytes);
    if (e == hipSuccess)
        e = hipMemcpy(c->d_meta, empty.data(), h.meta_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMalloc((void**)&S->d_chunk_meta, 512 * sizeof(uint2));
    if (e != hipSuccess) {
        vxrt::free_world(c);
        return bad(VXRT_ERR_HIP, std::string("stream tables: ") + hipGetErrorString(e));
    }
    c->nslots = pool_capacity_bricks;
    vxrt::fill_view(c, h.factor, cd);
    c->has_world = true;
    c->stream = S;
    return VXRT_OK;
}

int vxrt_stream_focus(vxrt_ctx* c, const float focus[3], float radius, vxrt_stream_stats* out)
{
    if (!c || !focus || !vxrt::StreamPolicy::focus_valid(focus, radius))
        return fail(VXRT_ERR_INVALID, "NULL argument, non-finite focus, or negative or NaN radius");
    StreamState* S = c->stream;
    if (!S)
        return fail(VXRT_ERR_NO_WORLD, "no streamed world (vxrt_stream_open)");
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());  // no launch may read the tables while chunks come and go
    StreamDeviceIO io(c, S);
    vxrt::StreamPolicy::Result r;
    const int rc = S->P.focus(focus, radius, S->brick_bytes, io, r);
    // whether or not the call got through: the table updates and re-ordered bricks made so far are in place before any
    // launch -- on any stream -- reads them
    const hipError_t e = hipDeviceSynchronize();
    if (rc)
        return rc;
    if (e != hipSuccess)
        return fail(VXRT_ERR_HIP, std::string("hipDeviceSynchronize: ") + hipGetErrorString(e));
    if (out) {
        out->chunks_total = S->P.nchunks;
        out->chunks_occupied = S->P.chunks_occupied;
        out->chunks_resident = S->P.chunks_resident;
        out->bricks_resident = S->P.bricks_resident;
        out->chunks_loaded = r.loaded;
        out->chunks_evicted = r.evicted;
        out->chunks_missing = r.missing;
        out->bytes_read = r.bytes;
    }
    return VXRT_OK;
}

int vxrt_stream_resident(vxrt_ctx* c, uint8_t* flags, uint64_t n_chunks)
{
    if (!c || !flags)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (!c->stream)
        return fail(VXRT_ERR_NO_WORLD, "no streamed world (vxrt_stream_open)");
    if (n_chunks != c->stream->P.nchunks)
        return fail(VXRT_ERR_INVALID, "one flag per 8x8x8 tile of the coarse grid");
    for (uint64_t ch = 0; ch < n_chunks; ++ch)
        flags[ch] = c->stream->P.chunks[ch].base >= 0 ? 1 : 0;
    return VXRT_OK;
}

int vxrt_stream_close(vxrt_ctx* c)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (!c->stream)
        return VXRT_OK;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());
    vxrt::free_world(c);  // drops the stream state with the tables
    return VXRT_OK;
}

}  // extern "C"

// ---- voxel editing (include/vxrt.h): host side of the two kernels of vxrt_edit.hip -----------------------------------------
namespace vxrt {

// the pool to `capacity` bricks: a new allocation with the allocator's slack, the live slots copied, the old one freed.
// Called with the device idle.  On failure nothing has changed.
static int grow_pool(vxrt_ctx* c, uint64_t capacity)
{
    const uint64_t bw = c->view.brick_words;
    void* alloc = nullptr;
    uint64_t alloc_bytes = 0;
    uint32_t* pool = nullptr;
    hipError_t e = alloc_pool(bw, capacity, &alloc, &alloc_bytes, &pool);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(VXRT_ERR_NOMEM, std::string("brick pool growth to ") + std::to_string(capacity) + " bricks: " + hipGetErrorString(e));
    }
    if (c->nslots)
        e = hipMemcpy(pool, c->d_pool, c->nslots * bw * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(alloc);
        return fail(VXRT_ERR_HIP, std::string("brick pool growth: ") + hipGetErrorString(e));
    }
    (void)hipFree(c->pool_alloc);
    c->pool_alloc = alloc;
    c->pool_alloc_bytes = alloc_bytes;
    c->d_pool = pool;
    c->pool_capacity_slots = capacity;
    const int cd[3] = {c->view.cx, c->view.cy, c->view.cz};
    fill_view(c, c->view.f, cd);  // pool, pool_end, pool_lo, pool_hi follow the new allocation
    return VXRT_OK;
}

// the touched brick cells: the union of the ops' clipped brick boxes, deduplicated, in HBM cell order (ops: edit ops or
// stamps, anything with a clipped voxel box lo / hi)
template <class Op>
static void edit_cells(const std::vector<Op>& ops, int f, int cx, int cz, uint64_t ncells, std::vector<uint32_t>& cells)
{
    uint64_t total = 0;
    for (const Op& op : ops) {
        uint64_t v = 1;
        for (int a = 0; a < 3; ++a)
            v *= (uint64_t)(op.hi[a] / f - op.lo[a] / f + 1);
        total += v;
    }
    cells.clear();
    if (total <= ncells) {  // the usual case: a list of the boxes' cells, sorted
        cells.reserve(total);
        for (const Op& op : ops)
            for (int y = op.lo[1] / f; y <= op.hi[1] / f; ++y)
                for (int z = op.lo[2] / f; z <= op.hi[2] / f; ++z)
                    for (int x = op.lo[0] / f; x <= op.hi[0] / f; ++x)
                        cells.push_back((uint32_t)hbm_index(x, y, z, cx, cz));
        std::sort(cells.begin(), cells.end());
        cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    } else {  // boxes that overlap more than the world holds: one flag per cell
        std::vector<uint8_t> mark(ncells, 0);
        for (const Op& op : ops)
            for (int y = op.lo[1] / f; y <= op.hi[1] / f; ++y)
                for (int z = op.lo[2] / f; z <= op.hi[2] / f; ++z)
                    for (int x = op.lo[0] / f; x <= op.hi[0] / f; ++x)
                        mark[hbm_index(x, y, z, cx, cz)] = 1;
        for (uint64_t i = 0; i < ncells; ++i)
            if (mark[i])
                cells.push_back((uint32_t)i);
    }
}

// The host tail of an edit call, shared by vxrt_edit_voxels and vxrt_edit_stamps: the device synchronised, the touched
// cells' scratch reserved, the per-brick kernel (`launch`: the ops in, images, extents and {old slot, flags} out, in
// k_edit_bricks' format), the flags read back, the slot plan, pool growth, k_edit_commit, and the rollback of the free
// list when a step after planning fails.  `ops`: the validated, clipped ops as the kernel reads them (copied as bytes).
template <class Op, class Launch>
static int edit_run(vxrt_ctx* c, const std::vector<Op>& ops, Launch launch, vxrt_edit_stats* out)
{
    const int f = c->view.f;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());  // no launch may read the tables while they change
    vxrt_edit_stats st{};
    auto finish = [&]() {
        st.pool_slots = c->nslots;
        st.pool_capacity = c->pool_capacity_slots;
        st.bricks_live = c->nslots - c->free_slots.size();
        if (out)
            *out = st;
        return VXRT_OK;
    };
    std::vector<uint32_t> cells;
    edit_cells(ops, f, c->view.cx, c->view.cz, c->ncells, cells);
    const uint32_t n = (uint32_t)cells.size();
    st.bricks_touched = n;
    if (n == 0)
        return finish();
    const uint64_t bw = c->view.brick_words;
    // device scratch: ops and cells in; images, extents and {old slot, flags} out; the plan in
    const size_t ops_bytes = ops.size() * sizeof(Op);
    hipError_t e = c->edit_in.reserve(ops_bytes + (size_t)n * 4);
    if (e == hipSuccess)
        e = c->edit_scratch.reserve((size_t)n * bw * 4);
    if (e == hipSuccess)
        e = c->edit_out.reserve((size_t)n * 12);
    if (e == hipSuccess)
        e = c->edit_plan.reserve((size_t)n * 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(VXRT_ERR_NOMEM, std::string("edit scratch for ") + std::to_string(n) + " bricks: " + hipGetErrorString(e));
    }
    unsigned char* in = static_cast<unsigned char*>(c->edit_in.p);
    const Op* d_ops = reinterpret_cast<const Op*>(in);
    const uint32_t* d_cells = reinterpret_cast<const uint32_t*>(in + ops_bytes);
    uint32_t* d_img = static_cast<uint32_t*>(c->edit_scratch.p);
    uint2* d_info = static_cast<uint2*>(c->edit_out.p);
    uint32_t* d_ext = reinterpret_cast<uint32_t*>(d_info + n);
    {
        std::vector<unsigned char> host_in(ops_bytes + (size_t)n * 4);
        memcpy(host_in.data(), ops.data(), ops_bytes);
        memcpy(host_in.data() + ops_bytes, cells.data(), (size_t)n * 4);
        VX_HIP(hipMemcpy(in, host_in.data(), host_in.size(), hipMemcpyHostToDevice));
    }
    VX_HIP(launch(d_cells, n, d_ops, (uint32_t)ops.size(), d_img, d_ext, d_info));
    std::vector<uint2> info(n);
    VX_HIP(hipMemcpy(info.data(), d_info, (size_t)n * sizeof(uint2), hipMemcpyDeviceToHost));
    std::vector<uint32_t> old_slot(n);
    std::vector<uint8_t> flags(n);
    for (uint32_t i = 0; i < n; ++i) {
        old_slot[i] = info[i].x;
        flags[i] = (uint8_t)info[i].y;
    }
    EditPlan P;
    edit_plan_slots(old_slot.data(), flags.data(), n, c->free_slots, c->nslots, P);  // (undone below on failure)
    if (P.changed == 0)  // no voxel changed: the tables stay untouched
        return finish();
    int rc = VXRT_OK;
    if (P.nslots >= (1ull << 32) - 2)
        rc = fail(VXRT_ERR_NOMEM, "brick slots exhausted (32-bit slot numbers)");
    else if (P.nslots > c->pool_capacity_slots)
        rc = grow_pool(c, edit_grown_capacity(c->pool_capacity_slots, P.nslots));
    if (rc) {
        edit_plan_undo(P, c->free_slots);
        return rc;
    }
    uint32_t* d_new = static_cast<uint32_t*>(c->edit_plan.p);
    uint32_t* d_zero = d_new + n;
    std::vector<uint32_t> plan(P.new_slot);
    plan.insert(plan.end(), P.zero.begin(), P.zero.end());
    e = hipMemcpy(d_new, plan.data(), plan.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = edit_commit(d_cells, d_new, n, d_zero, (uint32_t)P.zero.size(), d_img, d_ext, c->d_pool, c->d_meta, c->d_coarse, f);
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        edit_plan_undo(P, c->free_slots);
        return fail(VXRT_ERR_HIP, std::string("edit commit: ") + hipGetErrorString(e));
    }
    c->nslots = P.nslots;
    c->edited = true;
    st.bricks_created = P.created;
    st.bricks_freed = P.freed;
    return finish();
}

// ---- what the calls on the resident world share (edits, stamps, reads, collision, islands, navigation, distance) -------

// the checks every call on the resident world makes after its argument checks, in the order of include/vxrt.h: a world
// resident, and not a streamed one (`verb`: what the call would do to it)
static int world_ready(const vxrt_ctx* c, const char* verb)
{
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    if (c->stream)
        return fail(VXRT_ERR_INVALID, std::string("a streamed world (vxrt_stream_open) is a cache: it is not ") + verb);
    return VXRT_OK;
}

// origin + dims of a box within int32 on every axis (`what`: the message's subject)
static int box_in_range(const int32_t origin[3], const int32_t dims[3], const char* what)
{
    for (int k = 0; k < 3; ++k)
        if ((int64_t)origin[k] + dims[k] > INT32_MAX)
            return fail(VXRT_ERR_INVALID, std::string(what) + ": origin + dims beyond 2^31 - 1");
    return VXRT_OK;
}

// the resident world as the query kernels read it
static CollideWorld query_world(const vxrt_ctx* c)
{
    const int cd[3] = {c->view.cx, c->view.cy, c->view.cz};
    return query_world(c->d_meta, c->d_pool, c->view.f, cd);
}

// the device memory of a _host call: one allocation, cut into sections that start on 256-byte boundaries, freed on every path
struct HostScratch {
    char* base = nullptr;
    size_t off[8] = {};
    ~HostScratch() { (void)hipFree(base); }
    // sections of these sizes in bytes (at most 8); the allocation's error is also cleared from hipGetLastError
    hipError_t alloc(std::initializer_list<size_t> bytes)
    {
        size_t total = 0, k = 0;
        for (size_t b : bytes) {
            off[k++] = total;
            total += section_up(b);
        }
        const hipError_t e = hipMalloc((void**)&base, total);
        if (e != hipSuccess)
            (void)hipGetLastError();
        return e;
    }
    template <class T>
    T* at(int k) const { return reinterpret_cast<T*>(base + off[k]); }
};

}  // namespace vxrt

extern "C" {

int vxrt_edit_voxels(vxrt_ctx* c, const vxrt_edit_op* ops, uint32_t n_ops, vxrt_edit_stats* out)
{
    using vxrt::EditOpDev;
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (n_ops > vxrt::kEditMaxOps)
        return fail(VXRT_ERR_INVALID, "more than VXRT_EDIT_MAX_OPS ops in one call");
    if (!ops && n_ops)
        return fail(VXRT_ERR_INVALID, "ops is NULL");
    const int f = c->has_world ? c->view.f : 1;
    const int X = c->has_world ? c->view.cx * f : 1, Y = c->has_world ? c->view.cy * f : 1, Z = c->has_world ? c->view.cz * f : 1;
    std::vector<EditOpDev> dev;
    dev.reserve(n_ops);
    for (uint32_t k = 0; k < n_ops; ++k) {
        EditOpDev d;
        bool noop = false;
        if (vxrt::edit_prepare(ops[k].kind, ops[k].value, ops[k].a, ops[k].b, X, Y, Z, d, noop))
            return fail(VXRT_ERR_INVALID, "edit op " + std::to_string(k) +
                                              ": unknown kind, value not 0 / 1, negative radius or nonzero b[1] / b[2] on a sphere");
        if (!noop)
            dev.push_back(d);
    }
    if (int rc = vxrt::world_ready(c, "edited"))
        return rc;
    auto launch = [&](const uint32_t* d_cells, uint32_t n, const EditOpDev* d_ops, uint32_t nops, uint32_t* d_img,
                      uint32_t* d_ext, uint2* d_info) {
        return vxrt::edit_bricks(d_cells, n, d_ops, nops, c->d_meta, c->d_pool, d_img, d_ext, d_info, f, c->view.cx, c->view.cz);
    };
    return vxrt::edit_run(c, dev, launch, out);
}

uint64_t vxrt_region_words(const int32_t dims[3])
{
    return dims ? vxrt::region_words(dims) : 0;
}

int vxrt_read_region(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t* d_bits, void* stream)
{
    if (!c || !origin || !dims || !d_bits)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (vxrt::region_words(dims) == 0)
        return fail(VXRT_ERR_INVALID, "region dims: each at least 1, at most 2^36 voxels");
    if (int rc = vxrt::world_ready(c, "read"))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::read_region(vxrt::query_world(c), origin, dims, d_bits, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_read_region_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t* bits)
{
    if (!c || !origin || !dims || !bits)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    const uint64_t words = vxrt::region_words(dims);
    if (words == 0)
        return fail(VXRT_ERR_INVALID, "region dims: each at least 1, at most 2^36 voxels");
    if (int rc = vxrt::world_ready(c, "read"))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({words * 4}))
        return fail(VXRT_ERR_NOMEM, std::string("region read of ") + std::to_string(words) + " words: " + hipGetErrorString(e));
    uint32_t* d_bits = T.at<uint32_t>(0);
    VX_HIP(vxrt::read_region(vxrt::query_world(c), origin, dims, d_bits, nullptr));
    VX_HIP(hipMemcpy(bits, d_bits, words * 4, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

int vxrt_edit_stamps(vxrt_ctx* c, const vxrt_stamp* stamps, uint32_t n_stamps, vxrt_edit_stats* out)
{
    using vxrt::StampDev;
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (n_stamps > vxrt::kEditMaxOps)
        return fail(VXRT_ERR_INVALID, "more than VXRT_EDIT_MAX_OPS stamps in one call");
    if (!stamps && n_stamps)
        return fail(VXRT_ERR_INVALID, "stamps is NULL");
    const int f = c->has_world ? c->view.f : 1;
    const int X = c->has_world ? c->view.cx * f : 1, Y = c->has_world ? c->view.cy * f : 1, Z = c->has_world ? c->view.cz * f : 1;
    std::vector<StampDev> dev;
    dev.reserve(n_stamps);
    for (uint32_t k = 0; k < n_stamps; ++k) {
        const vxrt_stamp& s = stamps[k];
        StampDev d;
        bool noop = false;
        if (vxrt::stamp_prepare(s.d_bits, s.origin, s.dims, s.mode, s.reserved, X, Y, Z, d, noop))
            return fail(VXRT_ERR_INVALID, "stamp " + std::to_string(k) +
                                              ": unknown mode, nonzero reserved, d_bits NULL, or dims outside 1 .. 2^36 voxels");
        if (!noop)
            dev.push_back(d);
    }
    if (int rc = vxrt::world_ready(c, "edited"))
        return rc;
    auto launch = [&](const uint32_t* d_cells, uint32_t n, const StampDev* d_st, uint32_t nst, uint32_t* d_img,
                      uint32_t* d_ext, uint2* d_info) {
        return vxrt::stamp_bricks(d_cells, n, d_st, nst, c->d_meta, c->d_pool, d_img, d_ext, d_info, f, c->view.cx, c->view.cz);
    };
    return vxrt::edit_run(c, dev, launch, out);
}

// ---- box collision queries -------------------------------------------------------------------------------------------
static bool collide_order(const int32_t* order, int out[3])
{
    if (!order)
        return false;
    unsigned seen = 0;
    for (int k = 0; k < 3; ++k) {
        if (order[k] < 0 || order[k] > 2)
            return false;
        seen |= 1u << order[k];
        out[k] = order[k];
    }
    return seen == 7u;
}

int vxrt_move_boxes(vxrt_ctx* c, const vxrt_body* d_bodies, uint64_t n, const int32_t order[3], float* d_lohi_out,
                    uint32_t* d_flags_or_null, void* stream)
{
    int ord[3];
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (!collide_order(order, ord))
        return fail(VXRT_ERR_INVALID, "order must be a permutation of {0, 1, 2}");
    if (n == 0)
        return VXRT_OK;
    if (!d_bodies || !d_lohi_out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = vxrt::world_ready(c, "queried"))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::move_boxes(vxrt::query_world(c), (const float*)d_bodies, n, ord, d_lohi_out, d_flags_or_null,
                            (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_overlap_boxes(vxrt_ctx* c, const vxrt_body* d_bodies, uint64_t n, uint32_t* d_counts, uint32_t* d_flags_or_null,
                       void* stream)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (n == 0)
        return VXRT_OK;
    if (!d_bodies || !d_counts)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = vxrt::world_ready(c, "queried"))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::overlap_boxes(vxrt::query_world(c), (const float*)d_bodies, n, d_counts, d_flags_or_null, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_move_boxes_host(vxrt_ctx* c, const vxrt_body* bodies, uint64_t n, const int32_t order[3], float* lohi_out,
                         uint32_t* flags_or_null)
{
    int ord[3];
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (!collide_order(order, ord))
        return fail(VXRT_ERR_INVALID, "order must be a permutation of {0, 1, 2}");
    if (n == 0)
        return VXRT_OK;
    if (!bodies || !lohi_out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = vxrt::world_ready(c, "queried"))
        return rc;
    if (n > (1ull << 36))
        return fail(VXRT_ERR_INVALID, "too many bodies for one host call");
    VX_HIP(hipSetDevice(c->device));
    vxrt::HostScratch T;
    const size_t bb = (size_t)n * sizeof(vxrt_body), ob = (size_t)n * 24, fb = (size_t)n * 4;
    if (hipError_t e = T.alloc({bb, ob, fb}))
        return fail(VXRT_ERR_NOMEM, std::string("move_boxes_host: ") + hipGetErrorString(e));
    float *d_bodies = T.at<float>(0), *d_lohi = T.at<float>(1);
    uint32_t* d_flags = T.at<uint32_t>(2);
    VX_HIP(hipMemcpy(d_bodies, bodies, bb, hipMemcpyHostToDevice));
    VX_HIP(vxrt::move_boxes(vxrt::query_world(c), d_bodies, n, ord, d_lohi, d_flags, nullptr));
    VX_HIP(hipMemcpy(lohi_out, d_lohi, ob, hipMemcpyDeviceToHost));
    if (flags_or_null)
        VX_HIP(hipMemcpy(flags_or_null, d_flags, fb, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

int vxrt_overlap_boxes_host(vxrt_ctx* c, const vxrt_body* bodies, uint64_t n, uint32_t* counts, uint32_t* flags_or_null)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (n == 0)
        return VXRT_OK;
    if (!bodies || !counts)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = vxrt::world_ready(c, "queried"))
        return rc;
    if (n > (1ull << 36))
        return fail(VXRT_ERR_INVALID, "too many bodies for one host call");
    VX_HIP(hipSetDevice(c->device));
    vxrt::HostScratch T;
    const size_t bb = (size_t)n * sizeof(vxrt_body), cb = (size_t)n * 4;
    if (hipError_t e = T.alloc({bb, cb, cb}))
        return fail(VXRT_ERR_NOMEM, std::string("overlap_boxes_host: ") + hipGetErrorString(e));
    float* d_bodies = T.at<float>(0);
    uint32_t *d_counts = T.at<uint32_t>(1), *d_flags = T.at<uint32_t>(2);
    VX_HIP(hipMemcpy(d_bodies, bodies, bb, hipMemcpyHostToDevice));
    VX_HIP(vxrt::overlap_boxes(vxrt::query_world(c), d_bodies, n, d_counts, d_flags, nullptr));
    VX_HIP(hipMemcpy(counts, d_counts, cb, hipMemcpyDeviceToHost));
    if (flags_or_null)
        VX_HIP(hipMemcpy(flags_or_null, d_flags, cb, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- floating islands ------------------------------------------------------------------------------------------------
uint64_t vxrt_islands_workspace_bytes(const int32_t dims[3])
{
    vxrt::IslandsLayout L;
    return dims && vxrt::islands_layout(dims, L) ? L.total_bytes : 0;
}

// the checks both island calls make after their NULL checks, in the order of include/vxrt.h
static int islands_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t anchors)
{
    vxrt::IslandsLayout L;
    if (!vxrt::islands_layout(dims, L))
        return fail(VXRT_ERR_INVALID, "island box dims: each at least 1, at most 2^28 voxels");
    if (int rc = vxrt::box_in_range(origin, dims, "island box"))
        return rc;
    if (anchors & ~vxrt::kIslAnchorMask)
        return fail(VXRT_ERR_INVALID, "anchors: only VXRT_ISLAND_ANCHOR_* bits");
    return vxrt::world_ready(c, "queried");
}

int vxrt_find_islands(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t anchors, void* d_work,
                      uint32_t* d_floating, uint32_t* d_labels_or_null, vxrt_island* d_islands_or_null, uint32_t max_islands,
                      vxrt_island_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !d_work || !d_floating || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = islands_ready(c, origin, dims, anchors))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::find_islands(vxrt::query_world(c), origin, dims, anchors, d_work, d_floating, d_labels_or_null, d_islands_or_null,
                              max_islands, d_summary, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_find_islands_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t anchors, uint32_t* floating,
                           uint32_t* labels_or_null, vxrt_island* islands_or_null, uint32_t max_islands,
                           vxrt_island_summary* summary)
{
    if (!c || !origin || !dims || !floating || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = islands_ready(c, origin, dims, anchors))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::IslandsLayout L;
    vxrt::islands_layout(dims, L);
    const size_t fb = (size_t)vxrt::region_words(dims) * 4u, lb = labels_or_null ? (size_t)L.nvox * 4u : 0;
    const size_t tb = islands_or_null ? (size_t)max_islands * sizeof(vxrt_island) : 0;
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({L.total_bytes, fb, lb, tb, sizeof(vxrt_island_summary)}))
        return fail(VXRT_ERR_NOMEM, std::string("find_islands_host: ") + hipGetErrorString(e));
    uint32_t *d_float = T.at<uint32_t>(1), *d_lab = T.at<uint32_t>(2);
    vxrt_island* d_tab = T.at<vxrt_island>(3);
    vxrt_island_summary* d_sum = T.at<vxrt_island_summary>(4);
    VX_HIP(vxrt::find_islands(vxrt::query_world(c), origin, dims, anchors, T.base, d_float, labels_or_null ? d_lab : nullptr,
                              islands_or_null ? d_tab : nullptr, islands_or_null ? max_islands : 0u, d_sum, nullptr));
    VX_HIP(hipMemcpy(summary, d_sum, sizeof(vxrt_island_summary), hipMemcpyDeviceToHost));
    VX_HIP(hipMemcpy(floating, d_float, fb, hipMemcpyDeviceToHost));
    if (labels_or_null)
        VX_HIP(hipMemcpy(labels_or_null, d_lab, lb, hipMemcpyDeviceToHost));
    if (islands_or_null) {
        const size_t rows = summary->islands < max_islands ? summary->islands : max_islands;
        if (rows)
            VX_HIP(hipMemcpy(islands_or_null, d_tab, rows * sizeof(vxrt_island), hipMemcpyDeviceToHost));
    }
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- voxel piece queries ---------------------------------------------------------------------------------------------
// the checks both piece calls make after the NULL ctx, in the order of include/vxrt.h; fills A's pieces and launch shape
static int place_ready(const vxrt_piece* pieces, uint32_t n_pieces, vxrt::PlaceArgs& A)
{
    if (n_pieces < 1 || n_pieces > vxrt::kPlaceMaxPieces)
        return fail(VXRT_ERR_INVALID, "n_pieces: 1 .. VXRT_PLACE_MAX_PIECES");
    if (!pieces)
        return fail(VXRT_ERR_INVALID, "pieces is NULL");
    A.n_pieces = n_pieces;
    for (uint32_t k = 0; k < n_pieces; ++k)
        if (vxrt::piece_prepare(pieces[k].d_bits, pieces[k].dims, pieces[k].reserved, A.pieces[k]))
            return fail(VXRT_ERR_INVALID, "piece " + std::to_string(k) +
                                              ": bits NULL, nonzero reserved, a dim outside 1 .. 1024 or more than 2^24 voxels");
    vxrt::place_shape(A);
    return VXRT_OK;
}

int vxrt_place_pieces(vxrt_ctx* c, const vxrt_piece* pieces, uint32_t n_pieces, const vxrt_placement* d_placements, uint64_t n,
                      vxrt_placed* d_results, void* stream)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    vxrt::PlaceArgs A{};
    if (int rc = place_ready(pieces, n_pieces, A))
        return rc;
    if (n == 0)
        return VXRT_OK;
    if (!d_placements || !d_results)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = vxrt::world_ready(c, "queried"))
        return rc;
    A.W = vxrt::query_world(c);
    A.placements = (const int32_t*)d_placements;
    A.results = (uint32_t*)d_results;
    A.n = n;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::place_pieces(A, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_place_pieces_host(vxrt_ctx* c, const vxrt_piece* pieces, uint32_t n_pieces, const vxrt_placement* placements, uint64_t n,
                           vxrt_placed* results)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    vxrt::PlaceArgs A{};
    if (int rc = place_ready(pieces, n_pieces, A))
        return rc;
    if (n == 0)
        return VXRT_OK;
    if (!placements || !results)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = vxrt::world_ready(c, "queried"))
        return rc;
    if (n > (1ull << 36))
        return fail(VXRT_ERR_INVALID, "too many placements for one call");
    VX_HIP(hipSetDevice(c->device));
    // one allocation: the placements, the results, then every piece's words (each section on a 256-byte boundary)
    const size_t pb = (size_t)n * sizeof(vxrt_placement), rb = (size_t)n * sizeof(vxrt_placed);
    size_t off[vxrt::kPlaceMaxPieces], total = vxrt::section_up(pb) + vxrt::section_up(rb);
    for (uint32_t k = 0; k < n_pieces; ++k) {
        off[k] = total;
        total += vxrt::section_up((size_t)vxrt::region_words(pieces[k].dims) * 4u);
    }
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({total}))
        return fail(VXRT_ERR_NOMEM, std::string("place_pieces_host: ") + hipGetErrorString(e));
    vxrt_placement* d_pl = (vxrt_placement*)T.base;
    vxrt_placed* d_res = (vxrt_placed*)(T.base + vxrt::section_up(pb));
    VX_HIP(hipMemcpy(d_pl, placements, pb, hipMemcpyHostToDevice));
    for (uint32_t k = 0; k < n_pieces; ++k) {
        VX_HIP(hipMemcpy(T.base + off[k], pieces[k].d_bits, (size_t)vxrt::region_words(pieces[k].dims) * 4u, hipMemcpyHostToDevice));
        A.pieces[k].bits = (const uint32_t*)(T.base + off[k]);
    }
    A.W = vxrt::query_world(c);
    A.placements = (const int32_t*)d_pl;
    A.results = (uint32_t*)d_res;
    A.n = n;
    VX_HIP(vxrt::place_pieces(A, nullptr));
    VX_HIP(hipMemcpy(results, d_res, rb, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- navigation fields -----------------------------------------------------------------------------------------------
uint64_t vxrt_nav_workspace_bytes(const int32_t dims[3], const vxrt_nav_agent* agent)
{
    vxrt::NavLayout L;
    return dims && agent && vxrt::nav_layout(dims, agent->width, agent->height, agent->climb, agent->drop, L) ? L.total_bytes : 0;
}

// the checks both field calls make after their NULL checks, in the order of include/vxrt.h
static int nav_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_nav_agent* ag, uint32_t n_goals,
                     uint32_t max_dist)
{
    vxrt::NavLayout L;
    if (!vxrt::nav_agent_ok(ag->width, ag->height, ag->climb, ag->drop))
        return fail(VXRT_ERR_INVALID, "nav agent: 1 <= width <= 8, 1 <= height <= 32, 0 <= climb <= 8, 0 <= drop <= 32");
    if (!vxrt::nav_layout(dims, ag->width, ag->height, ag->climb, ag->drop, L))
        return fail(VXRT_ERR_INVALID, "nav box dims: each at least 1, at most 2^28 cells");
    if (int rc = vxrt::box_in_range(origin, dims, "nav box"))
        return rc;
    if (max_dist < 1 || max_dist > vxrt::kNavMaxDist)
        return fail(VXRT_ERR_INVALID, "nav max_dist: 1 .. 2^24");
    if (n_goals > vxrt::kNavMaxGoals)
        return fail(VXRT_ERR_INVALID, "nav goals: at most VXRT_NAV_MAX_GOALS");
    return vxrt::world_ready(c, "queried");
}

int vxrt_nav_field(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_nav_agent* agent,
                   const int32_t* d_goals, uint32_t n_goals, uint32_t max_dist, void* d_work, uint32_t* d_walkable,
                   uint8_t* d_next, uint32_t* d_dist_or_null, vxrt_nav_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !agent || !d_work || !d_walkable || !d_next || !d_summary || (!d_goals && n_goals))
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = nav_ready(c, origin, dims, agent, n_goals, max_dist))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    if (vxrt::stream_capturing((hipStream_t)stream))  // (include/vxrt.h, "Stream capture": refused before anything is enqueued)
        return fail(VXRT_ERR_INVALID, "stream capture: vxrt_nav_field reads a termination flag on the host every few levels and cannot be captured");
    VX_HIP(vxrt::nav_field(vxrt::query_world(c), origin, dims, *agent, d_goals, n_goals, max_dist, d_work, d_walkable, d_next,
                           d_dist_or_null, d_summary, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_nav_field_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_nav_agent* agent,
                        const int32_t* goals, uint32_t n_goals, uint32_t max_dist, uint32_t* walkable, uint8_t* next,
                        uint32_t* dist_or_null, vxrt_nav_summary* summary)
{
    if (!c || !origin || !dims || !agent || !walkable || !next || !summary || (!goals && n_goals))
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = nav_ready(c, origin, dims, agent, n_goals, max_dist))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::NavLayout L;
    vxrt::nav_layout(dims, agent->width, agent->height, agent->climb, agent->drop, L);
    const size_t wb = (size_t)L.nb * 4u, nb = L.nvox, db = dist_or_null ? (size_t)L.nvox * 4u : 0, gb = (size_t)n_goals * 12u;
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({L.total_bytes, wb, nb, db, gb, sizeof(vxrt_nav_summary)}))
        return fail(VXRT_ERR_NOMEM, std::string("nav_field_host: ") + hipGetErrorString(e));
    uint32_t *d_walk = T.at<uint32_t>(1), *d_dist = T.at<uint32_t>(3);
    uint8_t* d_next = T.at<uint8_t>(2);
    int32_t* d_goals = T.at<int32_t>(4);
    vxrt_nav_summary* d_sum = T.at<vxrt_nav_summary>(5);
    if (n_goals)
        VX_HIP(hipMemcpy(d_goals, goals, gb, hipMemcpyHostToDevice));
    VX_HIP(vxrt::nav_field(vxrt::query_world(c), origin, dims, *agent, d_goals, n_goals, max_dist, T.base, d_walk, d_next,
                           dist_or_null ? d_dist : nullptr, d_sum, nullptr));
    VX_HIP(hipMemcpy(summary, d_sum, sizeof(vxrt_nav_summary), hipMemcpyDeviceToHost));
    VX_HIP(hipMemcpy(walkable, d_walk, wb, hipMemcpyDeviceToHost));
    VX_HIP(hipMemcpy(next, d_next, nb, hipMemcpyDeviceToHost));
    if (dist_or_null)
        VX_HIP(hipMemcpy(dist_or_null, d_dist, db, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

int vxrt_nav_paths(vxrt_ctx* c, const vxrt_nav_field_desc* field, const int32_t* d_starts, uint64_t n, uint32_t max_steps,
                   int32_t* d_cells_or_null, uint32_t* d_lengths, uint32_t* d_status, void* stream)
{
    if (!c || !field || !field->d_next || !d_starts || !d_lengths || !d_status)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    vxrt::NavLayout L;
    const vxrt_nav_agent& ag = field->agent;
    if (!vxrt::nav_layout(field->dims, ag.width, ag.height, ag.climb, ag.drop, L))
        return fail(VXRT_ERR_INVALID, "nav field: bad dims or agent");
    if (int rc = vxrt::box_in_range(field->origin, field->dims, "nav field"))
        return rc;
    if (max_steps > vxrt::kNavMaxSteps)
        return fail(VXRT_ERR_INVALID, "nav paths: max_steps above 65535");
    if (n == 0)
        return VXRT_OK;
    VX_HIP(hipSetDevice(c->device));
    vxrt::NavPathArgs P{};
    P.next = field->d_next;
    P.starts = d_starts;
    P.cells = d_cells_or_null;
    P.lengths = d_lengths;
    P.status = d_status;
    P.n = n;
    P.max_steps = max_steps;
    for (int k = 0; k < 3; ++k) {
        P.o[k] = field->origin[k];
        P.d[k] = field->dims[k];
    }
    P.climb = ag.climb;
    P.drop = ag.drop;
    VX_HIP(vxrt::nav_paths(P, (hipStream_t)stream));
    return VXRT_OK;
}

// ---- distance fields -------------------------------------------------------------------------------------------------
uint64_t vxrt_distance_workspace_bytes(const int32_t dims[3], uint32_t radius)
{
    vxrt::DistLayout L;
    return dims && vxrt::dist_layout(nullptr, dims, radius, L) ? L.total_bytes : 0;
}

// the checks both distance calls make after their NULL checks, in the order of include/vxrt.h
static int distance_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t radius, int32_t mode)
{
    vxrt::DistLayout L;
    if (radius < 1 || radius > vxrt::kDistMaxRadius)
        return fail(VXRT_ERR_INVALID, "distance radius: 1 .. VXRT_DIST_MAX_RADIUS");
    if (!vxrt::dist_layout(nullptr, dims, radius, L))
        return fail(VXRT_ERR_INVALID, "distance box dims: each at least 1, at most 2^28 voxels, the halo box at most 2^36");
    if (!vxrt::dist_layout(origin, dims, radius, L))
        return fail(VXRT_ERR_INVALID, "distance box: origin - radius or origin + dims + radius beyond int32");
    if (mode != VXRT_DIST_TO_SOLID && mode != VXRT_DIST_TO_EMPTY)
        return fail(VXRT_ERR_INVALID, "distance mode: VXRT_DIST_TO_SOLID or VXRT_DIST_TO_EMPTY");
    return vxrt::world_ready(c, "queried");
}

int vxrt_distance_field(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t radius, int32_t mode, void* d_work,
                        uint16_t* d_dist2, vxrt_distance_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !d_work || !d_dist2 || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = distance_ready(c, origin, dims, radius, mode))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::distance_field(vxrt::query_world(c), origin, dims, radius, (uint32_t)mode, d_work, d_dist2, d_summary,
                                (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_distance_field_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t radius, int32_t mode,
                             uint16_t* dist2, vxrt_distance_summary* summary)
{
    if (!c || !origin || !dims || !dist2 || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = distance_ready(c, origin, dims, radius, mode))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::DistLayout L;
    vxrt::dist_layout(origin, dims, radius, L);
    const size_t ob = (size_t)L.nvox * 2u;
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({L.total_bytes, ob, sizeof(vxrt_distance_summary)}))
        return fail(VXRT_ERR_NOMEM, std::string("distance_field_host: ") + hipGetErrorString(e));
    uint16_t* d_out = T.at<uint16_t>(1);
    vxrt_distance_summary* d_sum = T.at<vxrt_distance_summary>(2);
    VX_HIP(vxrt::distance_field(vxrt::query_world(c), origin, dims, radius, (uint32_t)mode, T.base, d_out, d_sum, nullptr));
    VX_HIP(hipMemcpy(summary, d_sum, sizeof(vxrt_distance_summary), hipMemcpyDeviceToHost));
    VX_HIP(hipMemcpy(dist2, d_out, ob, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- mesh voxelization -------------------------------------------------------------------------------------------------
uint64_t vxrt_voxelize_workspace_bytes(const int32_t dims[3], uint32_t n_triangles)
{
    vxrt::VoxLayout L;
    return dims && vxrt::vox_layout(dims, n_triangles, L) ? L.total_bytes : 0;
}

// the checks both voxelize calls make after their NULL checks, in the order of include/vxrt.h
static int voxelize_ready(const int32_t dims[3], uint32_t n_triangles, int32_t modes, const void* vertices, const void* triangles)
{
    vxrt::VoxLayout L;
    if (modes < 1 || modes > 3)
        return fail(VXRT_ERR_INVALID, "voxelize modes: VXRT_VOX_SURFACE, VXRT_VOX_SOLID or both");
    if (!vxrt::vox_layout(dims, 0, L))
        return fail(VXRT_ERR_INVALID, "voxelize dims: each 1 .. VXRT_VOX_MAX_DIM");
    if (n_triangles > vxrt::kVoxMaxTriangles)
        return fail(VXRT_ERR_INVALID, "voxelize: more than 2^24 triangles");
    if (n_triangles && (!vertices || !triangles))
        return fail(VXRT_ERR_INVALID, "voxelize: vertices or triangles NULL with n_triangles > 0");
    return VXRT_OK;
}

int vxrt_voxelize_mesh(vxrt_ctx* c, const int32_t* d_vertices, uint32_t n_vertices, const uint32_t* d_triangles, uint32_t n_triangles,
                       const int32_t dims[3], int32_t modes, void* d_work, uint32_t* d_bits, vxrt_voxelize_summary* d_summary,
                       void* stream)
{
    if (!c || !dims || !d_work || !d_bits || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = voxelize_ready(dims, n_triangles, modes, d_vertices, d_triangles))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::voxelize_mesh(d_vertices, n_vertices, d_triangles, n_triangles, dims, (uint32_t)modes, d_work, d_bits, d_summary,
                               c->cus * 8u, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_voxelize_mesh_host(vxrt_ctx* c, const int32_t* vertices, uint32_t n_vertices, const uint32_t* triangles,
                            uint32_t n_triangles, const int32_t dims[3], int32_t modes, uint32_t* bits,
                            vxrt_voxelize_summary* summary)
{
    if (!c || !dims || !bits || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = voxelize_ready(dims, n_triangles, modes, vertices, triangles))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::VoxLayout L;
    vxrt::vox_layout(dims, n_triangles, L);
    const size_t vb = n_triangles ? (size_t)n_vertices * 12u : 0, tb = (size_t)n_triangles * 12u, ob = (size_t)L.words * 4u;
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({L.total_bytes, ob, sizeof(vxrt_voxelize_summary), vb, tb}))
        return fail(VXRT_ERR_NOMEM, std::string("voxelize_mesh_host: ") + hipGetErrorString(e));
    uint32_t* d_out = T.at<uint32_t>(1);
    vxrt_voxelize_summary* d_sum = T.at<vxrt_voxelize_summary>(2);
    if (vb)
        VX_HIP(hipMemcpy(T.at<int32_t>(3), vertices, vb, hipMemcpyHostToDevice));
    if (tb)
        VX_HIP(hipMemcpy(T.at<uint32_t>(4), triangles, tb, hipMemcpyHostToDevice));
    VX_HIP(vxrt::voxelize_mesh(T.at<int32_t>(3), n_vertices, T.at<uint32_t>(4), n_triangles, dims, (uint32_t)modes, T.base, d_out,
                               d_sum, c->cus * 8u, nullptr));
    VX_HIP(hipMemcpy(summary, d_sum, sizeof(vxrt_voxelize_summary), hipMemcpyDeviceToHost));
    VX_HIP(hipMemcpy(bits, d_out, ob, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- surface extraction --------------------------------------------------------------------------------------------------
uint64_t vxrt_surface_workspace_bytes(const int32_t dims[3])
{
    vxrt::SurfLayout L;
    return dims && vxrt::surf_layout(nullptr, dims, L) ? L.total_bytes : 0;
}

// the checks both surface calls make after their NULL checks, in the order of include/vxrt.h
static int surface_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], int32_t mode, const void* quads,
                         uint32_t capacity, const void* vertices, const void* triangles)
{
    vxrt::SurfLayout L;
    if (mode != VXRT_SURF_CAP && mode != VXRT_SURF_OPEN)
        return fail(VXRT_ERR_INVALID, "surface mode: VXRT_SURF_CAP or VXRT_SURF_OPEN");
    if (!vxrt::surf_layout(nullptr, dims, L))
        return fail(VXRT_ERR_INVALID, "surface box dims: each 1 .. VXRT_SURF_MAX_DIM, at most 2^28 voxels");
    if (!vxrt::surf_layout(origin, dims, L))
        return fail(VXRT_ERR_INVALID, "surface box: origin - 1 or origin + dims + 1 beyond int32");
    if (!quads && capacity)
        return fail(VXRT_ERR_INVALID, "surface: quads NULL with capacity_quads > 0");
    if (!vertices != !triangles)
        return fail(VXRT_ERR_INVALID, "surface: vertices and triangles are both NULL or both given");
    return vxrt::world_ready(c, "queried");
}

int vxrt_extract_surface(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], int32_t mode, void* d_work, vxrt_quad* d_quads,
                         uint32_t capacity_quads, int32_t* d_vertices, uint32_t* d_triangles, vxrt_surface_summary* d_summary,
                         void* stream)
{
    if (!c || !origin || !dims || !d_work || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = surface_ready(c, origin, dims, mode, d_quads, capacity_quads, d_vertices, d_triangles))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::extract_surface(vxrt::query_world(c), origin, dims, (uint32_t)mode, d_work, d_quads, capacity_quads, d_vertices,
                                 d_triangles, d_summary, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_extract_surface_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], int32_t mode, vxrt_quad* quads,
                              uint32_t capacity_quads, int32_t* vertices, uint32_t* triangles, vxrt_surface_summary* summary)
{
    if (!c || !origin || !dims || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = surface_ready(c, origin, dims, mode, quads, capacity_quads, vertices, triangles))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::SurfLayout L;
    vxrt::surf_layout(origin, dims, L);
    const size_t cap = vertices && capacity_quads > vxrt::kSurfMaxIndexed ? vxrt::kSurfMaxIndexed : capacity_quads;
    const size_t qb = cap * sizeof(vxrt_quad), vb = vertices ? cap * 48u : 0, tb = vertices ? cap * 24u : 0;
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({L.total_bytes, sizeof(vxrt_surface_summary), qb, vb, tb}))
        return fail(VXRT_ERR_NOMEM, std::string("extract_surface_host: ") + hipGetErrorString(e));
    vxrt_surface_summary* d_sum = T.at<vxrt_surface_summary>(1);
    VX_HIP(vxrt::extract_surface(vxrt::query_world(c), origin, dims, (uint32_t)mode, T.base, cap ? T.at<vxrt_quad>(2) : nullptr,
                                 (uint32_t)cap, vb ? T.at<int32_t>(3) : nullptr, tb ? T.at<uint32_t>(4) : nullptr, d_sum, nullptr));
    VX_HIP(hipMemcpy(summary, d_sum, sizeof(vxrt_surface_summary), hipMemcpyDeviceToHost));
    const size_t n = summary->written;  // only the records written come back: nothing past them is touched
    if (n)
        VX_HIP(hipMemcpy(quads, T.at<vxrt_quad>(2), n * sizeof(vxrt_quad), hipMemcpyDeviceToHost));
    if (n && vertices) {
        VX_HIP(hipMemcpy(vertices, T.at<int32_t>(3), n * 48u, hipMemcpyDeviceToHost));
        VX_HIP(hipMemcpy(triangles, T.at<uint32_t>(4), n * 24u, hipMemcpyDeviceToHost));
    }
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- occupancy LOD ----------------------------------------------------------------------------------------------------------
uint64_t vxrt_lod_workspace_bytes(const int32_t dims[3], uint32_t shift)
{
    vxrt::LodLayout L;
    return dims && vxrt::lod_layout(nullptr, dims, shift, L) ? L.total_bytes : 0;
}

// the checks both LOD calls make after their NULL checks, in the order of include/vxrt.h
static int lod_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t shift, uint32_t threshold)
{
    vxrt::LodLayout L;
    if (shift < 1u || shift > VXRT_LOD_MAX_SHIFT)
        return fail(VXRT_ERR_INVALID, "lod shift: 1 .. VXRT_LOD_MAX_SHIFT");
    if (!vxrt::lod_threshold_ok(shift, threshold))
        return fail(VXRT_ERR_INVALID, "lod threshold: 1 .. f^3 with f = 1 << shift");
    if (!vxrt::lod_layout(nullptr, dims, shift, L))
        return fail(VXRT_ERR_INVALID, "lod dims: each at least 1, the source box dims << shift at most 2^32 voxels");
    if (!vxrt::lod_layout(origin, dims, shift, L))
        return fail(VXRT_ERR_INVALID, "lod box: origin + (dims << shift) beyond 2^31 - 1");
    return vxrt::world_ready(c, "queried");
}

int vxrt_downsample_region(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t shift, uint32_t threshold,
                           void* d_work, uint32_t* d_bits, uint16_t* d_counts_or_null, vxrt_lod_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !d_work || !d_bits || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = lod_ready(c, origin, dims, shift, threshold))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::downsample_region(vxrt::query_world(c), origin, dims, shift, threshold, d_work, d_bits, d_counts_or_null, d_summary,
                                   (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_downsample_region_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], uint32_t shift, uint32_t threshold,
                                uint32_t* bits, uint16_t* counts_or_null, vxrt_lod_summary* summary)
{
    if (!c || !origin || !dims || !bits || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = lod_ready(c, origin, dims, shift, threshold))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::LodLayout L;
    vxrt::lod_layout(origin, dims, shift, L);
    const size_t bb = 4u * (size_t)vxrt::region_words(dims), cells = (size_t)dims[0] * L.rows, cb = counts_or_null ? 2u * cells : 0;
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({L.total_bytes, sizeof(vxrt_lod_summary), bb, cb}))
        return fail(VXRT_ERR_NOMEM, std::string("downsample_region_host: ") + hipGetErrorString(e));
    VX_HIP(vxrt::downsample_region(vxrt::query_world(c), origin, dims, shift, threshold, T.base, T.at<uint32_t>(2),
                                   cb ? T.at<uint16_t>(3) : nullptr, T.at<vxrt_lod_summary>(1), nullptr));
    VX_HIP(hipMemcpy(summary, T.at<vxrt_lod_summary>(1), sizeof(vxrt_lod_summary), hipMemcpyDeviceToHost));
    VX_HIP(hipMemcpy(bits, T.at<uint32_t>(2), bb, hipMemcpyDeviceToHost));
    if (cb)
        VX_HIP(hipMemcpy(counts_or_null, T.at<uint16_t>(3), cb, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- light fields ----------------------------------------------------------------------------------------------------------
uint64_t vxrt_light_workspace_bytes(const int32_t dims[3], uint32_t channels)
{
    vxrt::LightLayout L;
    return dims && vxrt::light_layout(nullptr, dims, channels, L) ? L.total_bytes : 0;
}

// the checks both light calls make after their NULL checks, in the order of include/vxrt.h
static int light_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const void* emitters, uint32_t n_emitters,
                       uint32_t channels)
{
    vxrt::LightLayout L;
    if (channels < 1u || channels > (VXRT_LIGHT_SKY | VXRT_LIGHT_BLOCK))
        return fail(VXRT_ERR_INVALID, "light channels: VXRT_LIGHT_SKY, VXRT_LIGHT_BLOCK or both");
    if (n_emitters > VXRT_LIGHT_MAX_EMITTERS)
        return fail(VXRT_ERR_INVALID, "light: more than VXRT_LIGHT_MAX_EMITTERS emitters");
    if (!emitters && n_emitters && (channels & VXRT_LIGHT_BLOCK))
        return fail(VXRT_ERR_INVALID, "light: emitters NULL with n_emitters > 0 and the block channel");
    if (!vxrt::light_layout(nullptr, dims, channels, L))
        return fail(VXRT_ERR_INVALID, "light box dims: each at least 1, at most 2^28 voxels, the halo box at most 2^36");
    if (!vxrt::light_layout(origin, dims, channels, L))
        return fail(VXRT_ERR_INVALID, "light box: origin - 14 or origin + dims + 14 beyond int32");
    return vxrt::world_ready(c, "queried");
}

int vxrt_light_field(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const int32_t* d_emitters, uint32_t n_emitters,
                     uint32_t channels, void* d_work, uint8_t* d_levels, vxrt_light_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !d_work || !d_levels || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = light_ready(c, origin, dims, d_emitters, n_emitters, channels))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::light_field(vxrt::query_world(c), origin, dims, channels, d_emitters, n_emitters, d_work, d_levels, d_summary,
                             (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_light_field_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const int32_t* emitters, uint32_t n_emitters,
                          uint32_t channels, uint8_t* levels, vxrt_light_summary* summary)
{
    if (!c || !origin || !dims || !levels || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = light_ready(c, origin, dims, emitters, n_emitters, channels))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::LightLayout L;
    vxrt::light_layout(origin, dims, channels, L);
    const size_t ob = L.nvox, eb = (channels & VXRT_LIGHT_BLOCK) ? (size_t)n_emitters * 16u : 0;
    vxrt::HostScratch T;
    if (hipError_t e = T.alloc({L.total_bytes, ob, sizeof(vxrt_light_summary), eb}))
        return fail(VXRT_ERR_NOMEM, std::string("light_field_host: ") + hipGetErrorString(e));
    if (eb)
        VX_HIP(hipMemcpy(T.at<int32_t>(3), emitters, eb, hipMemcpyHostToDevice));
    VX_HIP(vxrt::light_field(vxrt::query_world(c), origin, dims, channels, T.at<int32_t>(3), n_emitters, T.base, T.at<uint8_t>(1),
                             T.at<vxrt_light_summary>(2), nullptr));
    VX_HIP(hipMemcpy(summary, T.at<vxrt_light_summary>(2), sizeof(vxrt_light_summary), hipMemcpyDeviceToHost));
    VX_HIP(hipMemcpy(levels, T.at<uint8_t>(1), ob, hipMemcpyDeviceToHost));
    VX_HIP(hipDeviceSynchronize());
    return VXRT_OK;
}

// ---- frame denoiser ----------------------------------------------------------------------------------------------------
uint64_t vxrt_denoise_workspace_bytes(uint32_t W, uint32_t H) { return vxrt::denoise_workspace_bytes(W, H); }

int vxrt_frame_guides(vxrt_ctx* c, uint32_t W, uint32_t H, const float origin[3], const float fwd[3], const float up[3],
                      const float right[3], int32_t ortho, const int64_t* d_hit_aov, uint32_t* d_keys, void* stream)
{
    // the order of include/vxrt.h
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (!c->has_world)
        return fail(VXRT_ERR_INVALID, "frame guides: no world resident (its extents decode the hit index)");
    if (!vxrt::denoise_frame_ok(W, H))
        return fail(VXRT_ERR_INVALID, "frame guides: 1 <= W, H <= 65535 and W * H <= 2^26");
    if (!origin || !fwd || !up || !right || !d_hit_aov || !d_keys)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    const int64_t X = c->view.X, Y = c->view.Y, Z = (int64_t)c->view.cz * c->view.f;
    if (X > (int64_t)vxrt::kDnMaxAxis || Y > (int64_t)vxrt::kDnMaxAxis || Z > (int64_t)vxrt::kDnMaxAxis)
        return fail(VXRT_ERR_INVALID, "frame guides: a world axis longer than 2^24 voxels");
    VX_HIP(hipSetDevice(c->device));
    vxrt::RenderArgs A;
    memset(&A, 0, sizeof(A));
    A.W.X = (int)X;
    A.W.Y = (int)Y;
    camera_args(c, W, H, A);
    A.ortho = ortho ? 1 : 0;
    A.origin = vxrt::f3{origin[0], origin[1], origin[2]};
    A.fwd = vxrt::f3{fwd[0], fwd[1], fwd[2]};
    A.up = vxrt::f3{up[0], up[1], up[2]};
    A.right = vxrt::f3{right[0], right[1], right[2]};
    A.hit_aov = (long long*)d_hit_aov;
    VX_HIP(vxrt::frame_guides(A, (uint32_t)Z, d_keys, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_denoise_frame(vxrt_ctx* c, uint32_t W, uint32_t H, const float* d_color_in, const uint32_t* d_keys,
                       const vxrt_denoise_params* params, void* d_work, float* d_color_out, void* d_fb_or_null, void* stream)
{
    // the order of include/vxrt.h
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (!vxrt::denoise_frame_ok(W, H))
        return fail(VXRT_ERR_INVALID, "denoise: 1 <= W, H <= 65535 and W * H <= 2^26");
    if (!params || params->struct_size != sizeof(vxrt_denoise_params))
        return fail(VXRT_ERR_INVALID, "vxrt_denoise_params missing or size mismatch");
    if (params->iterations < 1 || params->iterations > vxrt::kDnMaxIterations)
        return fail(VXRT_ERR_INVALID, "denoise iterations: 1 .. 6");
    if (!(params->color_scale >= 0.0f))
        return fail(VXRT_ERR_INVALID, "denoise color_scale: negative or NaN");
    if (!d_color_in || !d_keys || !d_work || !d_color_out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::denoise_frame(W, H, d_color_in, d_keys, params->iterations, params->color_scale, d_work, d_color_out,
                               d_fb_or_null, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_edit_reserve(vxrt_ctx* c, uint64_t capacity_bricks)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (int rc = vxrt::world_ready(c, "edited"))
        return rc;
    if (capacity_bricks >= (1ull << 32) - 2)
        return fail(VXRT_ERR_INVALID, "capacity beyond 32-bit slot numbers");
    if (capacity_bricks <= c->pool_capacity_slots)
        return VXRT_OK;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(hipDeviceSynchronize());
    return vxrt::grow_pool(c, capacity_bricks);
}

}  // extern "C"
