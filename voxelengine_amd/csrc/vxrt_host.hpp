// vxrt_host.hpp -- what the translation units of the host side share (vxrt_api.hip, vxrt_api_file.hip, vxrt_api_query.hip,
// vxrt_worldgen.hip): the context behind the C ABI's opaque vxrt_ctx, the error message of vxrt_last_error, the functions
// that own the world tables, the checks every call on the resident world makes, and the device scratch of the _host calls.
#pragma once

#include "vxrt_kernels.hpp"
#include "vxrt_region.hpp"  // (and with it include/vxrt.h)

#include <atomic>
#include <set>
#include <string>
#include <vector>

namespace vxrt { int fail(int code, const std::string& msg); }  // vxrt_last_error's message set, `code` returned (vxrt_api.hip)
using vxrt::fail;

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
    // the last read's deltas of the loop diagnostics vxrt_frame_stats has no field for (vxrt_loop_counters_get)
    unsigned long long loop_counters[3] = {};
    // Rings: queue heads (render tile counters / batch tickets) and per-view argument slots of multi-view launches.  A ring
    // entry carries the event of the launch that used it last; taking an entry that is still in flight waits for that launch
    // (launch 65 of 64 in flight, multi-view launch 17 of 16), so an entry is never shared by two live launches.
    std::atomic<unsigned> launch_seq{0};
    hipEvent_t counter_busy[64] = {};
    vxrt::ViewArgs* d_views = nullptr;
    std::atomic<unsigned> view_seq{0};
    hipEvent_t views_busy[16] = {};
    int batch_max_steps = vxrt::kMaxSteps;  // Raytrace's maxSteps for the batch API (vxrt_set_batch_max_steps)
    struct StreamState* stream = nullptr;   // chunk streaming (vxrt_stream_*, vxrt_api_file.hip), or NULL
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

// ---- the world tables (vxrt_api.hip) ---------------------------------------------------------------------------------------
int check_shape(int factor, const int cd[3]);  // shared by upload, the brickmap file and the device builder
void fill_view(vxrt_ctx* c, int factor, const int cd[3]);
int alloc_world(vxrt_ctx* c, int factor, const int cd[3], uint64_t pool_slots);  // (frees a previous world, streamed or not)
// alloc_world, and the world made resident with `nslots` bricks whose tables the caller fills
int adopt_world(vxrt_ctx* c, int factor, const int cd[3], uint64_t nslots, uint32_t** d_coarse, uint2** d_meta,
                uint32_t** d_pool);
void abandon_world(vxrt_ctx* c);  // frees the tables (of a world whose build or load failed half way) and the stream state
int grow_pool(vxrt_ctx* c, uint64_t capacity);
bool stream_capturing(hipStream_t stream);
void camera_args(const vxrt_ctx* c, uint32_t width, uint32_t height, RenderArgs& A);
void stream_drop(vxrt_ctx* c);  // closes the chunk stream of a streamed world (vxrt_api_file.hip)
int build_world_on_device(vxrt_ctx* c, int generator, int X, int Y, int Z, int factor);  // vxrt_worldgen.hip

// ---- what the calls on the resident world share (edits, stamps, reads and every query family) ----------------------------

// the checks every call on the resident world makes after its argument checks, in the order of include/vxrt.h: a world
// resident, and not a streamed one (`verb`: what the call would do to it)
inline int world_ready(const vxrt_ctx* c, const char* verb)
{
    if (!c->has_world)
        return fail(VXRT_ERR_NO_WORLD, "no world resident");
    if (c->stream)
        return fail(VXRT_ERR_INVALID, std::string("a streamed world (vxrt_stream_open) is a cache: it is not ") + verb);
    return VXRT_OK;
}

// origin + dims of a box within int32 on every axis (`what`: the message's subject)
inline int box_in_range(const int32_t origin[3], const int32_t dims[3], const char* what)
{
    for (int k = 0; k < 3; ++k)
        if ((int64_t)origin[k] + dims[k] > INT32_MAX)
            return fail(VXRT_ERR_INVALID, std::string(what) + ": origin + dims beyond 2^31 - 1");
    return VXRT_OK;
}

// the resident world as the query kernels read it
inline CollideWorld query_world(const vxrt_ctx* c)
{
    const int cd[3] = {c->view.cx, c->view.cy, c->view.cz};
    return query_world(c->d_meta, c->d_pool, c->view.f, cd);
}

// The device memory of a _host call: one allocation cut into sections that start on 256-byte boundaries, freed on every
// path.  A section is declared once, before alloc(), and named by the handle its declaration returns: the section's device
// pointer once alloc() has succeeded, nullptr for a section of no bytes (an absent optional buffer).  The first section
// declared is the allocation's base.
class HostScratch {
    struct Part {
        size_t off, bytes, stride;
        const void* src;       // in(): copied to the section by alloc()
        void* dst;             // out(): the section copied there by finish(), or NULL
        const uint32_t* rows;  // out_rows(): only *rows records of `stride` bytes come back, read when finish() gets there
    };
    char* base_ = nullptr;
    size_t total_ = 0;
    std::vector<Part> parts_;

public:
    template <class T>
    struct Section {
        char* const* base = nullptr;
        size_t off = 0, bytes = 0;
        operator T*() const { return bytes ? reinterpret_cast<T*>(*base + off) : nullptr; }
    };
    ~HostScratch() { (void)hipFree(base_); }

    template <class T>
    Section<T> add(size_t bytes, const T* src, T* dst, size_t stride = 0, const uint32_t* rows = nullptr)
    {
        parts_.push_back(Part{total_, bytes, stride, src, dst, rows});
        total_ += section_up(bytes);
        return Section<T>{&base_, parts_.back().off, bytes};
    }
    // a workspace, which the host neither fills nor reads; an input; an output (dst NULL: the launch gets it, nothing comes back)
    Section<void> work(size_t bytes) { return add<void>(bytes, nullptr, nullptr); }
    template <class T>
    Section<T> in(size_t bytes, const T* src) { return add<T>(bytes, src, nullptr); }
    template <class T>
    Section<T> out(size_t bytes, T* dst) { return add<T>(bytes, nullptr, dst); }
    // an output of which the launch reports how much it wrote: `rows` points into the destination of an out() declared
    // earlier (a summary); only that many records, at most the section, come back and nothing behind them is touched
    template <class T>
    Section<T> out_rows(size_t bytes, T* dst, size_t stride, const uint32_t* rows) { return add<T>(bytes, nullptr, dst, stride, rows); }

    // the allocation (refused: `code` with the message "`what`: ...", the error cleared from hipGetLastError), then the copies in
    int alloc(int code, const std::string& what)
    {
        const hipError_t e = hipMalloc((void**)&base_, total_);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(code, what + ": " + hipGetErrorString(e));
        }
        for (const Part& p : parts_)
            if (p.src && p.bytes)
                VX_HIP(hipMemcpy(base_ + p.off, p.src, p.bytes, hipMemcpyHostToDevice));
        return VXRT_OK;
    }

    // after the launch (on the NULL stream): the copies out in the order of declaration, then the device synchronised
    int finish()
    {
        for (const Part& p : parts_) {
            const size_t n = p.rows && (size_t)*p.rows * p.stride < p.bytes ? (size_t)*p.rows * p.stride : p.bytes;
            if (p.dst && n)
                VX_HIP(hipMemcpy(p.dst, base_ + p.off, n, hipMemcpyDeviceToHost));
        }
        VX_HIP(hipDeviceSynchronize());
        return VXRT_OK;
    }
};

}  // namespace vxrt
