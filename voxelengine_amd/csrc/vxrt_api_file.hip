// vxrt_api_file.hip -- the part of the C ABI (include/vxrt.h) that reads and writes brickmap files: vxrt_world_file_info,
// vxrt_save_world, vxrt_load_world, and chunk streaming from such a file (vxrt_stream_*).  No kernel is defined here: the
// re-ordering launches are vxrt_worldgen.hip's, the compacting gather vxrt_edit.hip's.
#include "vxrt_edit.hpp"
#include "vxrt_host.hpp"
#include "vxrt_stream.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

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

extern "C" {

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
        vxrt::abandon_world(c);
        return fail(VXRT_ERR_INVALID, std::string(path) + ": " + why);
    };
    auto bad_hip = [&](hipError_t e) {
        vxrt::abandon_world(c);
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
    auto drop = [&](int rc) {  // a failure whose message is set
        fclose(S->f);
        delete S;
        return rc;
    };
    auto bad = [&](int code, const std::string& why) { return drop(fail(code, why)); };
    int rc = read_header(f, path, S->h);
    if (rc)
        return drop(rc);
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
    if (rc)
        return drop(rc);
    std::vector<uint2> empty(h.ncells, make_uint2(VXRT_EMPTY_SLOT, 0u));
    hipError_t e = hipMemset(c->d_coarse, 0, h.coarse_bytes);
    if (e == hipSuccess)  // the cache pool starts as empty space, not as whatever the allocation held
        e = hipMemset(c->d_pool, 0, pool_capacity_bricks * S->brick_bytes);
    if (e == hipSuccess)
        e = hipMemcpy(c->d_meta, empty.data(), h.meta_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMalloc((void**)&S->d_chunk_meta, 512 * sizeof(uint2));
    if (e != hipSuccess) {
        vxrt::abandon_world(c);
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
    vxrt::abandon_world(c);  // drops the stream state with the tables
    return VXRT_OK;
}

}  // extern "C"
