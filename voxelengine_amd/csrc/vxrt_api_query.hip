// vxrt_api_query.hip -- the part of the C ABI (include/vxrt.h) that works on the resident world: the edit path (vxrt_edit_*),
// every query family with its _host twin, and the entry points of the frame denoiser, the temporal filter, the light on frames, the voxel materials and the sky on frames.  No kernel is defined here: each family's
// launcher is declared in its header and defined in its own .hip.
#include "vxrt_collide.hpp"
#include "vxrt_denoise.hpp"
#include "vxrt_dist.hpp"
#include "vxrt_edit.hpp"
#include "vxrt_host.hpp"
#include "vxrt_islands.hpp"
#include "vxrt_light.hpp"
#include "vxrt_light_frame.hpp"
#include "vxrt_lod.hpp"
#include "vxrt_material.hpp"
#include "vxrt_nav.hpp"
#include "vxrt_place.hpp"
#include "vxrt_reproject.hpp"
#include "vxrt_rule.hpp"
#include "vxrt_loose.hpp"
#include "vxrt_sky.hpp"
#include "vxrt_surface.hpp"
#include "vxrt_transform.hpp"
#include "vxrt_voxelize.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

// ---- voxel editing (include/vxrt.h): host side of the two kernels of vxrt_edit.hip -----------------------------------------
namespace vxrt {

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
    auto each_cell = [&](auto&& visit) {
        for (const Op& op : ops)
            for (int y = op.lo[1] / f; y <= op.hi[1] / f; ++y)
                for (int z = op.lo[2] / f; z <= op.hi[2] / f; ++z)
                    for (int x = op.lo[0] / f; x <= op.hi[0] / f; ++x)
                        visit(hbm_index(x, y, z, cx, cz));
    };
    cells.clear();
    if (total <= ncells) {  // the usual case: a list of the boxes' cells, sorted
        cells.reserve(total);
        each_cell([&](uint64_t i) { cells.push_back((uint32_t)i); });
        std::sort(cells.begin(), cells.end());
        cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    } else {  // boxes that overlap more than the world holds: one flag per cell
        std::vector<uint8_t> mark(ncells, 0);
        each_cell([&](uint64_t i) { mark[i] = 1; });
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
    const auto d_bits = T.out(words * 4, bits);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "region read of " + std::to_string(words) + " words"))
        return rc;
    VX_HIP(vxrt::read_region(vxrt::query_world(c), origin, dims, d_bits, nullptr));
    return T.finish();
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
    const auto d_bodies = T.in((size_t)n * sizeof(vxrt_body), (const float*)bodies);
    const auto d_lohi = T.out((size_t)n * 24, lohi_out);
    const auto d_flags = T.out((size_t)n * 4, flags_or_null);  // (the kernel writes the flags either way)
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "move_boxes_host"))
        return rc;
    VX_HIP(vxrt::move_boxes(vxrt::query_world(c), d_bodies, n, ord, d_lohi, d_flags, nullptr));
    return T.finish();
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
    const auto d_bodies = T.in((size_t)n * sizeof(vxrt_body), (const float*)bodies);
    const auto d_counts = T.out((size_t)n * 4, counts);
    const auto d_flags = T.out((size_t)n * 4, flags_or_null);  // (the kernel writes the flags either way)
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "overlap_boxes_host"))
        return rc;
    VX_HIP(vxrt::overlap_boxes(vxrt::query_world(c), d_bodies, n, d_counts, d_flags, nullptr));
    return T.finish();
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
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_island_summary), summary);
    const auto d_float = T.out((size_t)vxrt::region_words(dims) * 4u, floating);
    const auto d_lab = T.out(labels_or_null ? (size_t)L.nvox * 4u : 0, labels_or_null);
    // the table's rows: min(summary->islands, max_islands) come back, the caller's rows behind them stay untouched
    const auto d_tab = T.out_rows(islands_or_null ? (size_t)max_islands * sizeof(vxrt_island) : 0, islands_or_null,
                                  sizeof(vxrt_island), &summary->islands);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "find_islands_host"))
        return rc;
    VX_HIP(vxrt::find_islands(vxrt::query_world(c), origin, dims, anchors, d_work, d_float, d_lab, d_tab,
                              islands_or_null ? max_islands : 0u, d_sum, nullptr));
    return T.finish();
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
    // the placements, the results, then every piece's words
    vxrt::HostScratch T;
    const auto d_pl = T.in((size_t)n * sizeof(vxrt_placement), (const int32_t*)placements);
    const auto d_res = T.out((size_t)n * sizeof(vxrt_placed), (uint32_t*)results);
    vxrt::HostScratch::Section<uint32_t> d_bits[vxrt::kPlaceMaxPieces];
    for (uint32_t k = 0; k < n_pieces; ++k)
        d_bits[k] = T.in((size_t)vxrt::region_words(pieces[k].dims) * 4u, pieces[k].d_bits);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "place_pieces_host"))
        return rc;
    for (uint32_t k = 0; k < n_pieces; ++k)
        A.pieces[k].bits = d_bits[k];
    A.W = vxrt::query_world(c);
    A.placements = d_pl;
    A.results = d_res;
    A.n = n;
    VX_HIP(vxrt::place_pieces(A, nullptr));
    return T.finish();
}

// ---- stamp orientations ----------------------------------------------------------------------------------------------
// the orientation of the C ABI as the algebra of vxrt_transform.hpp holds it (the same layout); false for NULL or an invalid one
static bool orient_of(const vxrt_orientation* o, vxrt::Orient& out)
{
    if (!o)
        return false;
    out = vxrt::Orient{{o->axis[0], o->axis[1], o->axis[2]}, o->flip};
    return vxrt::orient_valid(out);
}

static int orient_out(const vxrt::Orient& r, vxrt_orientation* out)
{
    for (int k = 0; k < 3; ++k)
        out->axis[k] = r.axis[k];
    out->flip = r.flip;
    return VXRT_OK;
}

int vxrt_orientation_rotation(int axis, int quarter_turns, vxrt_orientation* out)
{
    vxrt::Orient r;
    if (!out || !vxrt::orient_rotation(axis, quarter_turns, r))
        return VXRT_ERR_INVALID;
    return orient_out(r, out);
}

int vxrt_orientation_compose(const vxrt_orientation* a, const vxrt_orientation* b, vxrt_orientation* out)
{
    vxrt::Orient x, y;
    if (!out || !orient_of(a, x) || !orient_of(b, y))
        return VXRT_ERR_INVALID;
    return orient_out(vxrt::orient_compose(x, y), out);
}

int vxrt_orientation_inverse(const vxrt_orientation* o, vxrt_orientation* out)
{
    vxrt::Orient x;
    if (!out || !orient_of(o, x))
        return VXRT_ERR_INVALID;
    return orient_out(vxrt::orient_inverse(x), out);
}

int vxrt_orientation_dims(const vxrt_orientation* o, const int32_t src_dims[3], int32_t dst_dims[3])
{
    vxrt::Orient x;
    if (!src_dims || !dst_dims || !orient_of(o, x))
        return VXRT_ERR_INVALID;
    vxrt::orient_dims(x, src_dims, dst_dims);
    return VXRT_OK;
}

int vxrt_orientation_voxel(const vxrt_orientation* o, const int32_t src_dims[3], const int32_t p[3], int32_t q[3])
{
    vxrt::Orient x;
    if (!src_dims || !p || !q || !orient_of(o, x))
        return VXRT_ERR_INVALID;
    vxrt::orient_voxel(x, src_dims, p, q);
    return VXRT_OK;
}

int vxrt_orientation_is_rotation(const vxrt_orientation* o)
{
    vxrt::Orient x;
    if (!orient_of(o, x))
        return VXRT_ERR_INVALID;
    return vxrt::orient_is_rotation(x) ? 1 : 0;
}

// the checks both transform calls make, in the order of include/vxrt.h; fills A but for the summary
static int transform_ready(vxrt_ctx* c, const uint32_t* src, const int32_t src_dims[3], const vxrt_orientation* o, uint32_t* dst,
                           vxrt::TransformArgs& A)
{
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    static const char* const what[] = {"", "NULL argument", "orientation: axis a permutation of {0, 1, 2}, flip below 8",
                                       "src_dims: each at least 1, at most 2^36 voxels",
                                       "more than VXRT_TRANSFORM_MAX_WORDS words in the source or the destination",
                                       "the source and the destination overlap"};
    vxrt::Orient x{};
    if (o)
        x = vxrt::Orient{{o->axis[0], o->axis[1], o->axis[2]}, o->flip};
    if (const int bad = vxrt::transform_check(src, src_dims, o ? &x : nullptr, dst, A))
        return fail(VXRT_ERR_INVALID, what[bad]);
    return VXRT_OK;
}

int vxrt_transform_stamp(vxrt_ctx* c, const uint32_t* d_src, const int32_t src_dims[3], const vxrt_orientation* o, uint32_t* d_dst,
                         vxrt_transform_summary* d_summary_or_null, void* stream)
{
    vxrt::TransformArgs A;
    if (int rc = transform_ready(c, d_src, src_dims, o, d_dst, A))
        return rc;
    A.summary = (uint32_t*)d_summary_or_null;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::transform_stamp(A, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_transform_stamp_host(vxrt_ctx* c, const uint32_t* src, const int32_t src_dims[3], const vxrt_orientation* o, uint32_t* dst,
                              vxrt_transform_summary* summary_or_null)
{
    vxrt::TransformArgs A;
    if (int rc = transform_ready(c, src, src_dims, o, dst, A))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::HostScratch T;
    const auto d_src = T.in(4u * (size_t)A.nsrc, src);
    const auto d_dst = T.out(4u * (size_t)A.ndst, dst);
    const auto d_sum = T.out(summary_or_null ? sizeof(vxrt_transform_summary) : 0, summary_or_null);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "transform_stamp_host"))
        return rc;
    A.src = d_src;
    A.dst = d_dst;
    A.summary = (uint32_t*)(vxrt_transform_summary*)d_sum;
    VX_HIP(vxrt::transform_stamp(A, nullptr));
    return T.finish();
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
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_nav_summary), summary);
    const auto d_walk = T.out((size_t)L.nb * 4u, walkable);
    const auto d_next = T.out((size_t)L.nvox, next);
    const auto d_dist = T.out(dist_or_null ? (size_t)L.nvox * 4u : 0, dist_or_null);
    const auto d_goals = T.in((size_t)n_goals * 12u, goals);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "nav_field_host"))
        return rc;
    VX_HIP(vxrt::nav_field(vxrt::query_world(c), origin, dims, *agent, d_goals, n_goals, max_dist, d_work, d_walk, d_next,
                           d_dist, d_sum, nullptr));
    return T.finish();
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
    if (!vxrt::dist_layout(origin, dims, radius, L))
        return fail(VXRT_ERR_INVALID, L.fault == vxrt::kBoxDims
                                          ? "distance box dims: each at least 1, at most 2^28 voxels, the halo box at most 2^36"
                                          : "distance box: origin - radius or origin + dims + radius beyond int32");
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
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_distance_summary), summary);
    const auto d_out = T.out((size_t)L.nvox * 2u, dist2);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "distance_field_host"))
        return rc;
    VX_HIP(vxrt::distance_field(vxrt::query_world(c), origin, dims, radius, (uint32_t)mode, d_work, d_out, d_sum, nullptr));
    return T.finish();
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
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_voxelize_summary), summary);
    const auto d_out = T.out((size_t)L.words * 4u, bits);
    const auto d_verts = T.in(n_triangles ? (size_t)n_vertices * 12u : 0, vertices);
    const auto d_tris = T.in((size_t)n_triangles * 12u, triangles);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "voxelize_mesh_host"))
        return rc;
    VX_HIP(vxrt::voxelize_mesh(d_verts, n_vertices, d_tris, n_triangles, dims, (uint32_t)modes, d_work, d_out, d_sum, c->cus * 8u,
                               nullptr));
    return T.finish();
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
    if (!vxrt::surf_layout(origin, dims, L))
        return fail(VXRT_ERR_INVALID, L.fault == vxrt::kBoxDims ? "surface box dims: each 1 .. VXRT_SURF_MAX_DIM, at most 2^28 voxels"
                                                                : "surface box: origin - 1 or origin + dims + 1 beyond int32");
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
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_surface_summary), summary);
    // only the summary->written records written come back: nothing past them is touched
    const auto d_quads = T.out_rows(cap * sizeof(vxrt_quad), quads, sizeof(vxrt_quad), &summary->written);
    const auto d_verts = T.out_rows(vertices ? cap * 48u : 0, vertices, 48u, &summary->written);
    const auto d_tris = T.out_rows(vertices ? cap * 24u : 0, triangles, 24u, &summary->written);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "extract_surface_host"))
        return rc;
    VX_HIP(vxrt::extract_surface(vxrt::query_world(c), origin, dims, (uint32_t)mode, d_work, d_quads, (uint32_t)cap, d_verts, d_tris,
                                 d_sum, nullptr));
    return T.finish();
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
    if (!vxrt::lod_layout(origin, dims, shift, L))
        return fail(VXRT_ERR_INVALID, L.fault == vxrt::kBoxDims ? "lod dims: each at least 1, the source box dims << shift at most 2^32 voxels"
                                                                : "lod box: origin + (dims << shift) beyond 2^31 - 1");
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
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_lod_summary), summary);
    const auto d_bits = T.out(4u * (size_t)vxrt::region_words(dims), bits);
    const auto d_counts = T.out(counts_or_null ? 2u * (size_t)dims[0] * L.rows : 0, counts_or_null);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "downsample_region_host"))
        return rc;
    VX_HIP(vxrt::downsample_region(vxrt::query_world(c), origin, dims, shift, threshold, d_work, d_bits, d_counts, d_sum, nullptr));
    return T.finish();
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
    if (!vxrt::light_layout(origin, dims, channels, L))
        return fail(VXRT_ERR_INVALID, L.fault == vxrt::kBoxDims
                                          ? "light box dims: each at least 1, at most 2^28 voxels, the halo box at most 2^36"
                                          : "light box: origin - 14 or origin + dims + 14 beyond int32");
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
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_light_summary), summary);
    const auto d_levels = T.out((size_t)L.nvox, levels);
    const auto d_emitters = T.in((channels & VXRT_LIGHT_BLOCK) ? (size_t)n_emitters * 16u : 0, emitters);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "light_field_host"))
        return rc;
    VX_HIP(vxrt::light_field(vxrt::query_world(c), origin, dims, channels, d_emitters, n_emitters, d_work, d_levels, d_sum, nullptr));
    return T.finish();
}

// ---- voxel rules -----------------------------------------------------------------------------------------------------------
uint64_t vxrt_rule_workspace_bytes(const int32_t dims[3], const vxrt_rule* rule)
{
    vxrt::RuleLayout L;
    if (!dims || !rule || vxrt::rule_check(*rule) != 0)
        return 0;
    return vxrt::rule_layout(nullptr, dims, vxrt::rule_halo(*rule), L) ? L.total_bytes : 0;
}

// the checks both rule calls make after their NULL checks, in the order of include/vxrt.h
static int rule_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_rule* rule, const void* mask)
{
    static const char* const what[] = {
        "", "vxrt_rule size mismatch", "rule neighbours: VXRT_RULE_N6, VXRT_RULE_N18 or VXRT_RULE_N26",
        "rule born / survive: a bit above the number of neighbours", "rule iterations: 1 .. VXRT_RULE_MAX_ITERATIONS",
        "rule scope: VXRT_RULE_BOX or VXRT_RULE_WORLD", "rule outside: 0 or 1", "rule reserved_: 0"};
    if (const int bad = vxrt::rule_check(*rule))
        return fail(VXRT_ERR_INVALID, what[bad]);
    if (mask && rule->scope == VXRT_RULE_WORLD)
        return fail(VXRT_ERR_INVALID, "rule: a mask with VXRT_RULE_WORLD");
    vxrt::RuleLayout L;
    if (!vxrt::rule_layout(origin, dims, vxrt::rule_halo(*rule), L))
        return fail(VXRT_ERR_INVALID, L.fault == vxrt::kBoxDims
                                          ? "rule box dims: each at least 1, at most 2^28 voxels, the halo box at most 2^36"
                                          : "rule box: origin - halo or origin + dims + halo beyond int32");
    return vxrt::world_ready(c, "queried");
}

int vxrt_apply_rule(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_rule* rule, const uint32_t* d_mask_or_null,
                    void* d_work, uint32_t* d_bits, vxrt_rule_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !rule || !d_work || !d_bits || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = rule_ready(c, origin, dims, rule, d_mask_or_null))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::apply_rule(vxrt::query_world(c), origin, dims, *rule, d_mask_or_null, d_work, d_bits, d_summary, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_apply_rule_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_rule* rule,
                         const uint32_t* mask_or_null, uint32_t* bits, vxrt_rule_summary* summary)
{
    if (!c || !origin || !dims || !rule || !bits || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = rule_ready(c, origin, dims, rule, mask_or_null))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::RuleLayout L;
    vxrt::rule_layout(origin, dims, vxrt::rule_halo(*rule), L);
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_rule_summary), summary);
    const auto d_bits = T.out(4u * (size_t)L.nb, bits);
    const auto d_mask = T.in(mask_or_null ? 4u * (size_t)L.nb : 0, mask_or_null);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "apply_rule_host"))
        return rc;
    VX_HIP(vxrt::apply_rule(vxrt::query_world(c), origin, dims, *rule, d_mask, d_work, d_bits, d_sum, nullptr));
    return T.finish();
}

// ---- loose voxels -----------------------------------------------------------------------------------------------------------
uint64_t vxrt_loose_workspace_bytes(const int32_t dims[3])
{
    vxrt::LooseLayout L;
    return dims && vxrt::loose_layout(nullptr, dims, L) ? L.total_bytes : 0;
}

// the checks both loose calls make after their NULL checks, in the order of include/vxrt.h
static int loose_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_loose* params)
{
    static const char* const what[] = {"", "vxrt_loose size mismatch", "loose material: VXRT_LOOSE_SAND or VXRT_LOOSE_WATER",
                                       "loose steps: 1 .. VXRT_LOOSE_MAX_STEPS", "loose edge: VXRT_LOOSE_WALL or VXRT_LOOSE_OPEN",
                                       "loose reserved_: 0"};
    if (const int bad = vxrt::loose_check(*params))
        return fail(VXRT_ERR_INVALID, what[bad]);
    vxrt::LooseLayout L;
    if (!vxrt::loose_layout(origin, dims, L))
        return fail(VXRT_ERR_INVALID, L.fault == vxrt::kBoxDims
                                          ? "loose box dims: each at least 1, at most 2^28 voxels, the halo box at most 2^36"
                                          : "loose box: origin - 1 or origin + dims + 1 beyond int32");
    return vxrt::world_ready(c, "queried");
}

int vxrt_loose_step(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_loose* params, const uint32_t* d_loose_in,
                    void* d_work, uint32_t* d_loose_out, vxrt_loose_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !params || !d_loose_in || !d_work || !d_loose_out || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = loose_ready(c, origin, dims, params))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    VX_HIP(vxrt::loose_step(vxrt::query_world(c), origin, dims, *params, d_loose_in, d_work, d_loose_out, d_summary, (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_loose_step_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_loose* params, const uint32_t* loose_in,
                         uint32_t* loose_out, vxrt_loose_summary* summary)
{
    if (!c || !origin || !dims || !params || !loose_in || !loose_out || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = loose_ready(c, origin, dims, params))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::LooseLayout L;
    vxrt::loose_layout(origin, dims, L);
    vxrt::HostScratch T;
    const auto d_work = T.work(L.total_bytes);
    const auto d_sum = T.out(sizeof(vxrt_loose_summary), summary);
    const auto d_out = T.out(4u * (size_t)L.nb, loose_out);
    const auto d_in = T.in(4u * (size_t)L.nb, loose_in);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "loose_step_host"))
        return rc;
    VX_HIP(vxrt::loose_step(vxrt::query_world(c), origin, dims, *params, d_in, d_work, d_out, d_sum, nullptr));
    return T.finish();
}

// ---- what the frame calls share ----------------------------------------------------------------------------------------
// the camera of a W x H frame as camera_ray reads it: the context's constants (camera_args), the camera kind and the pose;
// everything else of R zero
static void frame_camera(const vxrt_ctx* c, uint32_t W, uint32_t H, int32_t ortho, const float origin[3], const float fwd[3],
                         const float up[3], const float right[3], vxrt::RenderArgs& R)
{
    memset(&R, 0, sizeof(R));
    vxrt::camera_args(c, W, H, R);
    R.ortho = ortho ? 1 : 0;
    R.origin = vxrt::f3{origin[0], origin[1], origin[2]};
    R.fwd = vxrt::f3{fwd[0], fwd[1], fwd[2]};
    R.up = vxrt::f3{up[0], up[1], up[2]};
    R.right = vxrt::f3{right[0], right[1], right[2]};
}

static void frame_camera(const vxrt_ctx* c, uint32_t W, uint32_t H, int32_t ortho, const vxrt_camera_pose& p, vxrt::RenderArgs& R)
{
    frame_camera(c, W, H, ortho, p.origin, p.fwd, p.up, p.right, R);
}

// the checks of a frame stage that decodes hit indices against the resident world (world_ready's `verb`; `stage`: the
// message's subject): a world that is not streamed, and no axis longer than a face plane's 2^24
static int frame_world_ready(const vxrt_ctx* c, const char* verb, const char* stage)
{
    if (int rc = vxrt::world_ready(c, verb))
        return rc;
    const vxrt::CollideWorld Wd = vxrt::query_world(c);
    for (int k = 0; k < 3; ++k)
        if ((uint32_t)Wd.dim[k] > vxrt::kDnMaxAxis)
            return fail(VXRT_ERR_INVALID, std::string(stage) + ": a world axis longer than 2^24 voxels");
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
    frame_camera(c, W, H, ortho, origin, fwd, up, right, A);
    A.W.X = (int)X;
    A.W.Y = (int)Y;
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

// ---- temporal filter ---------------------------------------------------------------------------------------------------
int vxrt_reproject_frame(vxrt_ctx* c, uint32_t W, uint32_t H, const float* d_color_in, const uint32_t* d_keys,
                         const vxrt_history* d_hist_in_or_null, const uint32_t* d_keys_prev_or_null,
                         const vxrt_reproject_params* params, vxrt_history* d_hist_out, float* d_color_out_or_null, void* d_fb_or_null,
                         vxrt_reproject_summary* d_summary_or_null, void* stream)
{
    // the order of include/vxrt.h
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (!vxrt::denoise_frame_ok(W, H))
        return fail(VXRT_ERR_INVALID, "reproject: 1 <= W, H <= 65535 and W * H <= 2^26");
    if (!params || params->struct_size != sizeof(vxrt_reproject_params))
        return fail(VXRT_ERR_INVALID, "vxrt_reproject_params missing or size mismatch");
    if (!vxrt::reproject_history_ok(params->max_history) || params->reserved_ != 0)
        return fail(VXRT_ERR_INVALID, "reproject max_history: 1 .. 65535 (and reserved_ 0)");
    if (!vxrt::pose_finite(params->cur) || !vxrt::pose_finite(params->prev))
        return fail(VXRT_ERR_INVALID, "reproject: a camera pose with a non-finite component");
    if (!d_color_in || !d_keys || !d_hist_out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    VX_HIP(hipSetDevice(c->device));
    vxrt::RenderArgs R;
    frame_camera(c, W, H, params->ortho, params->cur, R);
    vxrt::ReprojectArgs A{};
    const bool history = d_hist_in_or_null && d_keys_prev_or_null;
    A.color_in = d_color_in;
    A.keys = d_keys;
    A.hist_in = history ? (const vxrt::RpRec*)d_hist_in_or_null : nullptr;
    A.keys_prev = history ? d_keys_prev_or_null : nullptr;
    A.hist_out = (vxrt::RpRec*)d_hist_out;
    A.color_out = d_color_out_or_null;
    A.fb = (uint32_t*)d_fb_or_null;
    A.summary = (uint32_t*)d_summary_or_null;
    A.W = W;
    A.H = H;
    A.ortho = R.ortho;
    A.max_history = (float)params->max_history;
    A.kx = R.kx;
    A.ky = R.ky;
    A.ortho_x = R.ortho_x;
    A.ortho_y = R.ortho_y;
    A.ratio = R.ratio;
    for (int k = 0; k < 3; ++k) {
        A.po[k] = params->prev.origin[k];
        A.pf[k] = params->prev.fwd[k];
        A.pu[k] = params->prev.up[k];
        A.pr[k] = params->prev.right[k];
    }
    VX_HIP(vxrt::reproject_frame(R, A, c->cus, (hipStream_t)stream));
    return VXRT_OK;
}

// ---- light on frames ---------------------------------------------------------------------------------------------------
int vxrt_light_frame(vxrt_ctx* c, uint32_t W, uint32_t H, const float* d_color_in, const uint32_t* d_keys, const int64_t* d_hit_aov,
                     const uint8_t* d_levels_or_null, const vxrt_light_frame_params* params, float* d_color_out, void* d_fb_or_null,
                     float* d_terms_or_null, vxrt_light_frame_summary* d_summary_or_null, void* stream)
{
    // the order of include/vxrt.h
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    static const char* const refusal[] = {"", "", "light frame: 1 <= W, H <= 65535 and W * H <= 2^26",
                                          "vxrt_light_frame_params missing or size mismatch",
                                          "light frame flags: VXRT_LF_SMOOTH | VXRT_LF_OCCLUSION, outside_level <= 0xFF (and reserved_ 0)",
                                          "light frame sky_floor: 0 .. 1",
                                          "light frame: a block_color or ao_curve entry that is negative or not finite",
                                          "light frame: a camera pose with a non-finite component",
                                          "light frame box: 1 <= box_dims[k], their product <= 2^28, box_origin + box_dims <= 2^31 - 1"};
    if (const int r = vxrt::light_frame_check(W, H, params))
        return fail(VXRT_ERR_INVALID, refusal[r]);
    if (!d_color_in || !d_keys || !d_hit_aov || !d_color_out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = frame_world_ready(c, "lit", "light frame"))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::RenderArgs R;
    frame_camera(c, W, H, params->ortho, params->cam, R);
    vxrt::LightFrameArgs A{};
    vxrt::light_frame_args(A, W, H, *params);
    A.color_in = d_color_in;
    A.keys = d_keys;
    A.hit = (const long long*)d_hit_aov;
    A.levels = d_levels_or_null;
    A.color_out = d_color_out;
    A.fb = (uint32_t*)d_fb_or_null;
    A.terms = d_terms_or_null;
    A.summary = (uint32_t*)d_summary_or_null;
    VX_HIP(vxrt::light_frame(R, A, vxrt::query_world(c), c->cus, (hipStream_t)stream));
    return VXRT_OK;
}

// ---- voxel materials ---------------------------------------------------------------------------------------------------
static const char* const kRulesRefusal[] = {"", "vxrt_material_rules missing or size mismatch", "material rules: n_bands 1 .. 8",
                                            "material rules: bands[0].y_from INT32_MIN, y_from ascending, top, under and deep "
                                            "1 .. 255, under_depth 0 .. 15",
                                            "material rules: reserved_ must be 0"};
static const char* const kPaintRefusal =
    "material paint box: 1 <= paint_dims[k], their product <= 2^28, paint_origin + paint_dims <= 2^31 - 1";

// the checks both field calls make after their NULL checks, in the order of include/vxrt.h
static int material_field_ready(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_material_rules* rules,
                                const void* paint)
{
    if (const int r = vxrt::material_rules_check(rules))
        return fail(VXRT_ERR_INVALID, kRulesRefusal[r]);
    if (paint && !vxrt::material_paint_ok(*rules))
        return fail(VXRT_ERR_INVALID, kPaintRefusal);
    if (const int r = vxrt::material_box_check(origin, dims))
        return fail(VXRT_ERR_INVALID, r == 1 ? "material box dims: each at least 1, at most 2^28 voxels"
                                             : "material box: origin + dims + 16 beyond 2^31 - 1");
    return vxrt::world_ready(c, "queried");
}

int vxrt_material_field(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_material_rules* rules,
                        const uint8_t* d_paint_or_null, uint8_t* d_materials, vxrt_material_summary* d_summary, void* stream)
{
    if (!c || !origin || !dims || !rules || !d_materials || !d_summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = material_field_ready(c, origin, dims, rules, d_paint_or_null))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::MaterialFieldArgs A{};
    vxrt::material_field_args(A, *rules, origin, dims, vxrt::material_field_segment(dims, c->cus), d_materials);
    A.paint = d_paint_or_null;
    A.summary = (uint32_t*)d_summary;
    VX_HIP(vxrt::material_field(A, vxrt::query_world(c), (hipStream_t)stream));
    return VXRT_OK;
}

int vxrt_material_field_host(vxrt_ctx* c, const int32_t origin[3], const int32_t dims[3], const vxrt_material_rules* rules,
                             const uint8_t* paint_or_null, uint8_t* materials, vxrt_material_summary* summary)
{
    if (!c || !origin || !dims || !rules || !materials || !summary)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = material_field_ready(c, origin, dims, rules, paint_or_null))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::HostScratch T;
    const auto d_sum = T.out(sizeof(vxrt_material_summary), summary);
    const auto d_mat = T.out((size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2], materials);
    const auto d_paint = T.in(paint_or_null ? (size_t)rules->paint_dims[0] * (size_t)rules->paint_dims[1] * (size_t)rules->paint_dims[2] : 0,
                              paint_or_null);
    if (int rc = T.alloc(VXRT_ERR_NOMEM, "material_field_host"))
        return rc;
    vxrt::MaterialFieldArgs A{};
    vxrt::material_field_args(A, *rules, origin, dims, vxrt::material_field_segment(dims, c->cus), d_mat);
    A.paint = d_paint;
    A.summary = (uint32_t*)(vxrt_material_summary*)d_sum;
    VX_HIP(vxrt::material_field(A, vxrt::query_world(c), nullptr));
    return T.finish();
}

int vxrt_material_frame(vxrt_ctx* c, uint32_t W, uint32_t H, const float* d_color_in, const uint32_t* d_keys, const int64_t* d_hit_aov,
                        const vxrt_material_rules* rules, const uint8_t* d_paint_or_null, const vxrt_material* d_palette,
                        const uint32_t* d_atlas_or_null, const vxrt_material_frame_params* params, float* d_color_out, void* d_fb_or_null,
                        uint8_t* d_material_aov_or_null, vxrt_material_frame_summary* d_summary_or_null, void* stream)
{
    // the order of include/vxrt.h
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    if (const int r = vxrt::material_frame_check(W, H, params, rules, d_paint_or_null != nullptr)) {
        static const char* const refusal[] = {"", "", "material frame: 1 <= W, H <= 65535 and W * H <= 2^26",
                                              "vxrt_material_frame_params missing or size mismatch",
                                              "material frame: n_tiles <= 4096, tile_shift <= 6 (and reserved_ 0)"};
        return fail(VXRT_ERR_INVALID, r <= 4 ? refusal[r] : r <= 8 ? kRulesRefusal[r - 4] : r == 9 ? "material frame: a camera pose with a non-finite component" : kPaintRefusal);
    }
    if (!d_color_in || !d_keys || !d_hit_aov || !d_palette || !d_color_out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    if (int rc = frame_world_ready(c, "queried", "material frame"))
        return rc;
    VX_HIP(hipSetDevice(c->device));
    vxrt::RenderArgs R;
    frame_camera(c, W, H, params->ortho, params->cam, R);
    vxrt::MaterialFrameArgs A{};
    A.rules = *rules;
    A.color_in = d_color_in;
    A.keys = d_keys;
    A.hit = (const long long*)d_hit_aov;
    A.paint = d_paint_or_null;
    A.palette = d_palette;
    A.atlas = d_atlas_or_null;
    A.color_out = d_color_out;
    A.fb = (uint32_t*)d_fb_or_null;
    A.aov = d_material_aov_or_null;
    A.summary = (uint32_t*)d_summary_or_null;
    A.W = W;
    A.H = H;
    A.n_tiles = params->n_tiles;
    A.tile_shift = params->tile_shift;
    VX_HIP(vxrt::material_frame(R, A, vxrt::query_world(c), c->cus, (hipStream_t)stream));
    return VXRT_OK;
}

// ---- sky on frames -----------------------------------------------------------------------------------------------------
int vxrt_sky_frame(vxrt_ctx* c, uint32_t W, uint32_t H, const float* d_color_in, const uint32_t* d_keys, const vxrt_sky_params* params,
                   float* d_color_out, void* d_fb_or_null, vxrt_sky_summary* d_summary_or_null, void* stream)
{
    // the order of include/vxrt.h
    if (!c)
        return fail(VXRT_ERR_INVALID, "ctx is NULL");
    static const char* const refusal[] = {"", "", "sky frame: 1 <= W, H <= 65535 and W * H <= 2^26",
                                          "vxrt_sky_params missing or size mismatch",
                                          "sky frame flags: VXRT_SKY_CLOUDS (and reserved_ 0)",
                                          "sky frame: a colour component that is negative or not finite",
                                          "sky frame: glow_log2 0 .. 8, octaves 1 .. 6",
                                          "sky frame: a scalar that is negative or not finite",
                                          "sky frame: fog_max and cloud_cover 0 .. 1",
                                          "sky frame: -1 <= cos_outer < cos_inner <= 1",
                                          "sky frame: a sun_dir that is zero or not finite",
                                          "sky frame: a camera pose with a non-finite component"};
    if (const int r = vxrt::sky_frame_check(W, H, params))
        return fail(VXRT_ERR_INVALID, refusal[r]);
    if (!d_color_in || !d_keys || !d_color_out)
        return fail(VXRT_ERR_INVALID, "NULL argument");
    VX_HIP(hipSetDevice(c->device));
    vxrt::RenderArgs R;
    frame_camera(c, W, H, params->ortho, params->cam, R);
    vxrt::SkyArgs A{};
    vxrt::sky_frame_args(A, W, H, *params);
    A.color_in = d_color_in;
    A.keys = d_keys;
    A.color_out = d_color_out;
    A.fb = (uint32_t*)d_fb_or_null;
    A.summary = (uint32_t*)d_summary_or_null;
    VX_HIP(vxrt::sky_frame(R, A, c->cus, (hipStream_t)stream));
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
