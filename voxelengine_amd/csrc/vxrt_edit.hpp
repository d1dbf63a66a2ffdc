// vxrt_edit.hpp -- voxel editing (include/vxrt.h, vxrt_edit_voxels): the pieces shared by the kernels of vxrt_edit.hip,
// the host side in vxrt_api_query.hip and the host harness of the tests (tests/tools/edit_check.cpp, through
// tests/tools/hoststub): op membership, the per-brick op filter, extent packing, and the slot plan.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <set>
#include <vector>

namespace vxrt {

constexpr uint32_t kEditMaxOps = 1024;  // VXRT_EDIT_MAX_OPS
constexpr uint32_t kEditKeep = 0xFFFFFFFEu;  // plan: the cell did not change, its record stays as it is

// an op as the kernels read it: validated, its voxel box clipped to the world (lo > hi on some axis: a no-op)
struct EditOpDev {
    int32_t kind, value;
    int32_t lo[3], hi[3];  // clipped voxel box, inclusive (a sphere's: centre +- radius)
    int32_t c[3];          // sphere centre (unclipped)
    int32_t pad_;
    uint64_t r2;           // sphere: radius^2
};

__host__ __device__ inline bool edit_in_box(const EditOpDev& op, int x, int y, int z)
{
    return x >= op.lo[0] && x <= op.hi[0] && y >= op.lo[1] && y <= op.hi[1] && z >= op.lo[2] && z <= op.hi[2];
}

// membership of voxel (x, y, z) (include/vxrt.h): inside the clipped box, and for a sphere inside the ball.  Inside the box
// every |d| <= r < 2^31, so the sum of the three squares stays below 3 * 2^62: exact in uint64.
__host__ __device__ inline bool edit_covers(const EditOpDev& op, int x, int y, int z)
{
    if (!edit_in_box(op, x, y, z))
        return false;
    if (op.kind == 0)
        return true;
    const int64_t dx = (int64_t)x - op.c[0], dy = (int64_t)y - op.c[1], dz = (int64_t)z - op.c[2];
    return (uint64_t)(dx * dx) + (uint64_t)(dy * dy) + (uint64_t)(dz * dz) <= op.r2;
}

// the op's box meets the brick's voxel box [b0, b0 + f - 1]^3
__host__ __device__ inline bool edit_meets_brick(const EditOpDev& op, const int b0[3], int f)
{
    for (int a = 0; a < 3; ++a)
        if (op.hi[a] < b0[a] || op.lo[a] > b0[a] + f - 1)
            return false;
    return true;
}

// the op covers every voxel of the brick: a box containing it, or a ball containing its eight corners (a ball is convex)
__host__ __device__ inline bool edit_covers_brick(const EditOpDev& op, const int b0[3], int f)
{
    for (int k = 0; k < 8; ++k)
        if (!edit_covers(op, b0[0] + ((k & 1) ? f - 1 : 0), b0[1] + ((k & 2) ? f - 1 : 0), b0[2] + ((k & 4) ? f - 1 : 0)))
            return false;
    return true;
}

// extents of a brick, packed as the cell records hold them (min x,y,z then max x,y,z, 5 bits each); empty = 0
__host__ __device__ inline uint32_t edit_pack_extents(const int mn[3], const int mx[3])
{
    if (mx[0] < 0)
        return 0u;
    return (uint32_t)mn[0] | ((uint32_t)mn[1] << 5) | ((uint32_t)mn[2] << 10) | ((uint32_t)mx[0] << 15) |
           ((uint32_t)mx[1] << 20) | ((uint32_t)mx[2] << 25);
}

// ---- host: op validation and clipping, slot plan -------------------------------------------------------------------
// 0 = valid; X, Y, Z = world voxels per axis.  *noop = the op cannot change any voxel.
inline int edit_prepare(int32_t kind, int32_t value, const int32_t a[3], const int32_t b[3], int X, int Y, int Z,
                        EditOpDev& out, bool& noop)
{
    if (!(kind == 0 || kind == 1) || !(value == 0 || value == 1))
        return -1;
    if (kind == 1 && (b[0] < 0 || b[1] != 0 || b[2] != 0))
        return -1;
    const int64_t dim[3] = {X, Y, Z};
    out = EditOpDev{};
    out.kind = kind;
    out.value = value;
    noop = false;
    for (int k = 0; k < 3; ++k) {
        int64_t lo = kind == 0 ? (int64_t)a[k] : (int64_t)a[k] - b[0];
        int64_t hi = kind == 0 ? (int64_t)b[k] : (int64_t)a[k] + b[0];
        lo = lo < 0 ? 0 : lo;
        hi = hi > dim[k] - 1 ? dim[k] - 1 : hi;
        if (lo > hi) {
            noop = true;
            lo = 1;
            hi = 0;
        }
        out.lo[k] = (int32_t)lo;
        out.hi[k] = (int32_t)hi;
        out.c[k] = a[k];
    }
    out.r2 = kind == 1 ? (uint64_t)b[0] * (uint64_t)b[0] : 0u;
    return 0;
}

// The slot plan of one edit call, from what k_edit_bricks reported per touched cell (cell order): the cell's old slot
// and its flags (bit 0: the new brick is non-empty, bit 1: it differs from the old one).  Deterministic: frees first,
// then every cell that becomes non-empty takes the lowest free slot (freed by this call or earlier), else the next slot
// past the high-water mark `nslots`.  `free_slots` is updated in place (edit_plan_undo puts it back: the cost of a call
// stays proportional to the bricks it touches, whatever the free list holds); P.nslots above the pool's capacity means
// the pool must grow.
struct EditPlan {
    std::vector<uint32_t> new_slot;  // per touched cell: kEditKeep, kEmptySlot (freed) or the brick's slot
    std::vector<uint32_t> zero;      // slots freed by this call and still free after it (ascending): zeroed
    std::vector<uint32_t> freed_now, taken;  // slots this call put on the free list / took from it
    uint64_t created = 0, freed = 0, changed = 0;
    uint64_t nslots = 0;             // high-water mark after the call
};

inline void edit_plan_slots(const uint32_t* old_slot, const uint8_t* flags, size_t n, std::set<uint32_t>& free_slots,
                            uint64_t nslots, EditPlan& P)
{
    constexpr uint32_t kEmpty = 0xFFFFFFFFu;
    P = EditPlan{};
    P.new_slot.assign(n, kEditKeep);
    std::vector<uint32_t>& freed_now = P.freed_now;
    std::vector<size_t> create;
    for (size_t i = 0; i < n; ++i) {
        if (!(flags[i] & 2u))
            continue;
        ++P.changed;
        const bool any = (flags[i] & 1u) != 0;
        if (old_slot[i] != kEmpty && !any) {
            P.new_slot[i] = kEmpty;
            free_slots.insert(old_slot[i]);
            freed_now.push_back(old_slot[i]);
            ++P.freed;
        } else if (old_slot[i] == kEmpty && any) {
            create.push_back(i);
        } else {
            P.new_slot[i] = old_slot[i];  // rewritten in place
        }
    }
    for (size_t i : create) {
        uint32_t s;
        if (!free_slots.empty()) {
            s = *free_slots.begin();
            free_slots.erase(free_slots.begin());
            P.taken.push_back(s);
        } else {
            s = (uint32_t)nslots++;
        }
        P.new_slot[i] = s;
        ++P.created;
    }
    for (uint32_t s : freed_now)
        if (free_slots.count(s))
            P.zero.push_back(s);
    std::sort(P.zero.begin(), P.zero.end());
    P.nslots = nslots;
}

// the free list as it was before edit_plan_slots made P (a call that fails after planning)
inline void edit_plan_undo(const EditPlan& P, std::set<uint32_t>& free_slots)
{
    for (uint32_t s : P.taken)
        free_slots.insert(s);
    for (uint32_t s : P.freed_now)  // (slots in use before the call: none of them was free)
        free_slots.erase(s);
}

// capacity after a growth that must hold `needed` slots: 1.5x the old capacity or more
inline uint64_t edit_grown_capacity(uint64_t capacity, uint64_t needed)
{
    const uint64_t g = capacity + (capacity + 1) / 2;
    return needed > g ? needed : g;
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_edit.hip
hipError_t edit_bricks(const uint32_t* cells, uint32_t n, const EditOpDev* ops, uint32_t nops, const uint2* meta,
                       const uint32_t* pool, uint32_t* scratch, uint32_t* ext, uint2* info, int f, int cx, int cz);
hipError_t edit_commit(const uint32_t* cells, const uint32_t* new_slot, uint32_t n, const uint32_t* zero, uint32_t nzero,
                       const uint32_t* scratch, const uint32_t* ext, uint32_t* pool, uint2* meta, uint32_t* coarse, int f);
hipError_t gather_bricks(const uint32_t* pool, const uint32_t* idx, uint32_t n, uint32_t* dst, int f);
#endif

}  // namespace vxrt
