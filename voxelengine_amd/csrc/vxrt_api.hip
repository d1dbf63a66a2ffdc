// vxrt_api.hip -- host side of the C ABI declared in include/vxrt.h.  Owns the HBM-resident world tables, the camera/lighting
// state the reference keeps in process globals (hFrameInfo / g_env, VoxelRT/Renderer.cu:24-25,89) and the render and batch
// launches.  The brickmap file and chunk streaming: vxrt_api_file.hip; edits, queries and the denoiser: vxrt_api_query.hip.
#include "vxrt_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>

static thread_local std::string g_last_error = "";

int vxrt::fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

namespace vxrt {

void abandon_world(vxrt_ctx* c)
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
    abandon_world(c);
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

// the pool to `capacity` bricks: a new allocation with the allocator's slack, the live slots copied, the old one freed.
// Called with the device idle (the edit calls, vxrt_api_query.hip).  On failure nothing has changed.
int grow_pool(vxrt_ctx* c, uint64_t capacity)
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

// Whether `stream` is being captured into a graph (include/vxrt.h, "Stream capture"); asked once per call.  The NULL
// stream is never asked: it cannot be captured, and asking while another stream captures is itself an error.
bool stream_capturing(hipStream_t stream)
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

// What camera_ray (vxrt_camera.hpp) reads of a launch besides the view: the frame size and getRayDirection's per-pixel
// constants (Renderer.cu:46,50-52), hoisted to the host.  One place for the render launches and vxrt_frame_guides, whose keys
// are defined by the renderer's own primary rays.
void camera_args(const vxrt_ctx* c, uint32_t width, uint32_t height, RenderArgs& A)
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
    vxrt::abandon_world(c);
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
        vxrt::abandon_world(c);
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
    vxrt::camera_args(c, width, height, A);
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
    c->loop_counters[0] = h[vxrt::kStatDbgCoRuns];
    c->loop_counters[1] = h[vxrt::kStatDbgCoStarts];
    c->loop_counters[2] = h[vxrt::kStatDbgEndBounce];
    return VXRT_OK;
}

int vxrt_loop_counters_get(vxrt_ctx* c, uint64_t* out, int32_t capacity)
{
    if (!c || !out || capacity < 0)
        return fail(VXRT_ERR_INVALID, "NULL argument or negative capacity");
    const int32_t n = capacity < 3 ? capacity : 3;
    for (int32_t i = 0; i < n; ++i)
        out[i] = c->loop_counters[i];
    return 3;
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
    vxrt::HostScratch T;
    const auto d_o = T.in((size_t)n * 12, origins), d_d = T.in((size_t)n * 12, dirs);
    const auto d_p = T.out((size_t)n * 12, pos), d_n = T.out((size_t)n * 12, normal);
    const auto d_s = T.out((size_t)n * 4, steps);
    const auto d_h = T.out((size_t)n, hit);  // (both given to the launch whether or not the caller wants them back)
    const auto d_v = T.out((size_t)n * 8, voxel);
    if (int rc = T.alloc(VXRT_ERR_HIP, "trace_batch_host: hipMalloc"))
        return rc;
    if (int rc = vxrt_trace_batch(c, d_o, d_d, n, d_p, d_n, d_s, d_h, d_v, stats, nullptr))
        return rc;
    return T.finish();
}

}  // extern "C"
