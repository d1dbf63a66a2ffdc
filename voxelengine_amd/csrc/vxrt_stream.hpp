// vxrt_stream.hpp -- the bookkeeping of chunk streaming (include/vxrt.h, vxrt_stream_*), host C++ only: the chunk table
// built from a brickmap file's coarse bits and cell records, the distance order, the radius test, the eviction scan and
// the first-fit pool allocator.  What a load or an eviction does to the file and the device goes through StreamIO:
// vxrt_api_file.hip implements it with the file reads, copies and re-ordering launches, tests/tools/stream_check.cpp with
// no-ops (and chunks whose read fails), so the policy that runs in the library is the one the host tests check against
// tests/ref_stream.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace vxrt {

constexpr uint32_t kStreamEmptySlot = 0xFFFFFFFFu;  // VXRT_EMPTY_SLOT

struct StreamCell {  // one 8-byte cell record of a brickmap file: pool slot or kStreamEmptySlot, packed extents
    uint32_t slot, extents;
};

// tight extents of an occupied cell's record: six 5-bit fields {min x,y,z, max x,y,z}, each inside the brick, min <= max,
// nothing above them (shared by vxrt_load_world and vxrt_stream_open)
inline bool extents_valid(uint32_t packed, int factor)
{
    if ((packed >> 30) != 0u)
        return false;
    for (int a = 0; a < 3; ++a) {
        const uint32_t lo = (packed >> (5 * a)) & 31u, hi = (packed >> (5 * (a + 3))) & 31u;
        if (hi >= (uint32_t)factor || lo > hi)
            return false;
    }
    return true;
}

// what a focus call does outside the bookkeeping; a nonzero return is a vxrt status that ends the call as it stands
struct StreamIO {
    // read chunk `ch`'s bricks (file slots first_slot .. first_slot + nbricks - 1) into the pool from brick `start` on
    virtual int load(uint32_t ch, uint32_t first_slot, uint32_t nbricks, uint64_t start) = 0;
    // write chunk `ch`'s 512 cell records and coarse bits: its bricks from `base` on in cell order, or all empty
    virtual int tables(uint32_t ch, bool resident, int64_t base) = 0;
    virtual ~StreamIO() {}
};

struct StreamPolicy {
    struct Chunk {
        uint32_t first_slot = 0, nbricks = 0;   // its run of bricks in the file
        int64_t base = -1;                      // first brick of its range in the device pool, or -1 = not resident
        float lo[3], hi[3];                     // its box in voxels
    };
    std::vector<Chunk> chunks;
    std::map<uint64_t, uint64_t> free_ranges;   // device pool: start -> length, in bricks
    uint64_t nchunks = 0, capacity = 0, bricks_resident = 0, chunks_resident = 0, chunks_occupied = 0;

    struct Result {
        uint64_t loaded = 0, evicted = 0, missing = 0, bytes = 0;
    };

    // the chunk table of a file's tables (tiled-linear: chunk ch = cells ch * 512 .. ch * 512 + 511) and an empty pool of
    // `capacity` bricks; returns NULL, or why the tables cannot be streamed
    const char* init(int factor, const int cdims[3], const uint32_t* coarse, const StreamCell* meta, uint64_t nslots,
                     uint64_t pool_capacity)
    {
        const uint64_t ncells = (uint64_t)cdims[0] * cdims[1] * cdims[2];
        nchunks = ncells / 512;
        chunks.assign(nchunks, Chunk());
        const int tw = cdims[0] / 8, th = cdims[1] / 8;
        uint32_t next_slot = 0;
        for (uint64_t ch = 0; ch < nchunks; ++ch) {
            Chunk& C = chunks[ch];
            C.first_slot = next_slot;
            for (uint64_t i = ch * 512; i < ch * 512 + 512; ++i) {
                const bool bit = (coarse[i >> 5] >> (i & 31)) & 1u;
                // slots run through the file in cell order (vxrt_save_world writes what the builders produce): a chunk's
                // bricks are ONE contiguous run
                if (bit ? meta[i].slot != next_slot : meta[i].slot != kStreamEmptySlot)
                    return "brick slots are not in cell order";
                if (bit && !extents_valid(meta[i].extents, factor))  // (what vxrt_load_world checks of a cell record)
                    return "brick extents outside the brick";
                if (bit) {
                    ++next_slot;
                    ++C.nbricks;
                }
            }
            const int tx = (int)(ch % tw), ty = (int)((ch / tw) % th), tz = (int)(ch / ((uint64_t)tw * th));
            const float e = 8.0f * (float)factor;
            C.lo[0] = tx * e; C.lo[1] = ty * e; C.lo[2] = tz * e;
            C.hi[0] = C.lo[0] + e; C.hi[1] = C.lo[1] + e; C.hi[2] = C.lo[2] + e;
            if (C.nbricks)
                chunks_occupied += 1;
        }
        if (next_slot != nslots)
            return "brick count does not match the coarse bits";
        capacity = pool_capacity;
        free_ranges.clear();
        free_ranges[0] = pool_capacity;
        return nullptr;
    }

    // a focus with a non-finite component, or a radius that is negative or NaN, is refused (+inf is a radius)
    static bool focus_valid(const float focus[3], float radius)
    {
        return std::isfinite(focus[0]) && std::isfinite(focus[1]) && std::isfinite(focus[2]) && radius >= 0.0f;
    }

    bool alloc(uint64_t n, uint64_t& start)
    {
        for (auto it = free_ranges.begin(); it != free_ranges.end(); ++it)
            if (it->second >= n) {  // first fit
                start = it->first;
                const uint64_t rest = it->second - n, at = it->first + n;
                free_ranges.erase(it);
                if (rest)
                    free_ranges[at] = rest;
                return true;
            }
        return false;
    }
    void release(uint64_t start, uint64_t n)
    {
        auto next = free_ranges.lower_bound(start);
        if (next != free_ranges.begin()) {  // merge with the range that ends where this one starts
            auto prev = std::prev(next);
            if (prev->first + prev->second == start) {
                start = prev->first;
                n += prev->second;
                free_ranges.erase(prev);
            }
        }
        if (next != free_ranges.end() && start + n == next->first) {
            n += next->second;
            free_ranges.erase(next);
        }
        free_ranges[start] = n;
    }

    // one vxrt_stream_focus on a valid focus: every occupied chunk within the radius made resident, nearest first, room
    // made by evicting resident chunks outside the radius, farthest first.  Returns VXRT_OK (0) with the counts in `r`, or
    // the first nonzero status of `io`: the loads and evictions made before it stay; a chunk whose load or table write
    // failed is not resident (its bricks go back to the pool), a chunk whose eviction's table write failed stays resident.
    int focus(const float focus[3], float radius, uint64_t brick_bytes, StreamIO& io, Result& r)
    {
        r = Result();
        // squared distance of the focus to every occupied chunk's box
        std::vector<std::pair<float, uint32_t>> order;
        order.reserve(chunks_occupied);
        for (uint64_t ch = 0; ch < nchunks; ++ch) {
            const Chunk& C = chunks[ch];
            if (!C.nbricks)
                continue;
            float d2 = 0.0f;
            for (int a = 0; a < 3; ++a) {
                const float d = focus[a] < C.lo[a] ? C.lo[a] - focus[a] : (focus[a] > C.hi[a] ? focus[a] - C.hi[a] : 0.0f);
                d2 += d * d;
            }
            order.emplace_back(d2, (uint32_t)ch);
        }
        std::stable_sort(order.begin(), order.end(), [](const std::pair<float, uint32_t>& a, const std::pair<float, uint32_t>& b) {
            return a.first < b.first;
        });
        const float r2 = radius * radius;
        size_t far = order.size();  // eviction candidates: from the far end of the order, outside the radius only
        for (size_t k = 0; k < order.size() && order[k].first <= r2; ++k) {
            const uint32_t ch = order[k].second;
            Chunk& C = chunks[ch];
            if (C.base >= 0)
                continue;
            uint64_t start = 0;
            bool ok = alloc(C.nbricks, start);
            while (!ok && far > 0) {  // make room: the farthest resident chunk outside the radius goes
                --far;
                if (order[far].first <= r2)
                    break;
                Chunk& V = chunks[order[far].second];
                if (V.base < 0)
                    continue;
                if (int rc = io.tables(order[far].second, false, -1))
                    return rc;
                release((uint64_t)V.base, V.nbricks);
                bricks_resident -= V.nbricks;
                chunks_resident -= 1;
                V.base = -1;
                r.evicted += 1;
                ok = alloc(C.nbricks, start);
            }
            if (!ok) {
                r.missing += 1;
                continue;
            }
            int rc = io.load(ch, C.first_slot, C.nbricks, start);
            if (rc == 0)
                rc = io.tables(ch, true, (int64_t)start);
            if (rc) {
                release(start, C.nbricks);
                return rc;
            }
            r.bytes += (uint64_t)C.nbricks * brick_bytes;
            C.base = (int64_t)start;
            bricks_resident += C.nbricks;
            chunks_resident += 1;
            r.loaded += 1;
        }
        return 0;
    }
};

}  // namespace vxrt
