// Host harness of the stamp orientations (voxelengine_amd/csrc/vxrt_transform.hpp: the plan, the per-lane work of the COPY
// and of the TRANSPOSE kernel, the butterfly round, the tally and its commit), compiled for the CPU through
// tests/tools/hoststub and run launch by launch, workgroup by workgroup and lane by lane.  The harness restates what the
// kernels of vxrt_transform.hip add around that code, which the GPU suite covers:
//   the stride loops     the workgroups walking the destination words (COPY) or the tiles (TRANSPOSE);
//   the LDS images       two arrays per workgroup, the phases of a tile run one after the other (the barriers);
//   the xor shuffles     the butterfly rounds over the array of a half-wave's 32 lane values, lane i exchanging with lane
//                        i ^ (16 >> round); the workgroup's reduction of the tallies as a loop over its 256 lanes;
//   k_transform_init     the summary's eight words from tr_summary_init.
// Every index the code forms into the source, the destination, the summary or an LDS image is checked against that array's
// size; every destination word must be stored exactly once; destination and summary carry guard words behind them; LDS
// words are poisoned between tiles.  Run by tests/test_transform_host.py, which compares the outputs with
// tests/ref_transform.py.
//
//   transform_check in.bin out.bin
//   in:  i32 sd[3], axis[3], flip, summary (0 / 1), groups (0: as planned, else the workgroups of the launch);
//        region_words(sd) u32 source words
//   out: 8 u32 summary (zeros without one), region_words(dd) u32 destination words
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>

static void tr_check(int array, uint64_t index);
#define VXRT_TRANSFORM_CHECK(array, index) tr_check(array, (uint64_t)(index))

#include "../../voxelengine_amd/csrc/vxrt_transform.hpp"
#include "hbm_world.h"
#include <vector>
using namespace vxrt;

static std::vector<uint8_t> g_stores;  // per destination word (the hook of kTrDst sits at the store alone)
static void tr_check(int array, uint64_t index)
{
    check_index(array, index);
    if (array == kTrDst && index < g_stores.size())
        g_stores[index]++;
}

static uint32_t lcg_state = 2463534242u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }

// the five rounds over the 32 lane values of a half-wave
static void butterfly(uint32_t v[32])
{
    for (uint32_t round = 0; round < 5u; ++round) {
        uint32_t n[32];
        for (uint32_t i = 0; i < 32u; ++i)
            n[i] = tr_combine(v[i], v[i ^ (16u >> round)], round, i);
        for (uint32_t i = 0; i < 32u; ++i)
            v[i] = n[i];
    }
}

// the workgroup's reduction and the commit of its first lane
static void commit_group(const TransformArgs& A, const TrTally* t)
{
    uint64_t n = 0;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    for (uint32_t l = 0; l < kTrLanes; ++l) {
        n += t[l].n;
        for (int k = 0; k < 3; ++k) {
            lo[k] = t[l].lo[k] < lo[k] ? t[l].lo[k] : lo[k];
            hi[k] = t[l].hi[k] > hi[k] ? t[l].hi[k] : hi[k];
        }
    }
    tr_commit(A, n, lo, hi);
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: transform_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[9];
    if (!in || fread(hd, 4, 9, in) != 9)
        return 2;
    const int32_t sd[3] = {hd[0], hd[1], hd[2]};
    const Orient o{{hd[3], hd[4], hd[5]}, (uint32_t)hd[6]};
    const bool tally = hd[7] != 0;

    // the butterfly against the definition: bit b of lane i afterwards = bit i of lane b before
    for (int trial = 0; trial < 64; ++trial) {
        uint32_t v[32], w[32];
        for (uint32_t i = 0; i < 32u; ++i)
            w[i] = v[i] = trial == 0 ? 1u << i : (trial == 1 ? (i == 5u ? 0xFFFFFFFFu : 0u) : lcg());
        butterfly(w);
        for (uint32_t i = 0; i < 32u; ++i)
            for (uint32_t b = 0; b < 32u; ++b)
                CHECK(((w[i] >> b) & 1u) == ((v[b] >> i) & 1u));
        uint32_t rev = 0u;
        for (uint32_t b = 0; b < 32u; ++b)
            rev |= ((v[3] >> b) & 1u) << (31u - b);
        CHECK(tr_brev(v[3]) == rev);
    }

    TransformArgs A;
    if (!orient_valid(o) || transform_plan(sd, o, A) != 0) {
        printf("outside the contract\n");
        return 2;
    }
    std::vector<uint32_t> src(A.nsrc);
    if (fread(src.data(), 4, src.size(), in) != src.size())
        return 2;
    fclose(in);
    const uint32_t guard = 0x5A5A5A5Au;
    std::vector<uint32_t> dst(A.ndst + 4u, guard), summary(kTrSumWords + 4u, guard);
    g_stores.assign(A.ndst, 0);
    g_size[kTrSrc] = A.nsrc;
    g_size[kTrDst] = A.ndst;
    g_size[kTrSum] = tally ? kTrSumWords : 0u;
    g_size[kTrLdsIn] = kTrLdsInWords;
    g_size[kTrLdsOut] = kTrLdsOutWords;
    A.src = src.data();
    A.dst = dst.data();
    A.summary = tally ? summary.data() : nullptr;
    int32_t dd[3];
    orient_dims(o, sd, dd);
    CHECK(dd[0] == A.dd[0] && dd[1] == A.dd[1] && dd[2] == A.dd[2] && A.ndst == region_words(dd));

    if (tally)  // k_transform_init
        for (uint32_t i = 0; i < kTrSumWords; ++i) {
            tr_check(kTrSum, i);
            summary[i] = tr_summary_init(i);
        }
    const uint32_t groups = hd[8] > 0 ? (uint32_t)hd[8] : transform_groups(A);
    CHECK(groups >= 1u && groups <= kTrMaxGroups);
    std::vector<TrTally> t(kTrLanes);
    if (A.axis[0] == 0) {  // k_transform_copy
        const uint64_t stride = (uint64_t)groups * kTrLanes;
        CHECK(hd[8] > 0 || stride >= A.ndst || groups == kTrMaxGroups);
        for (uint32_t g = 0; g < groups; ++g) {
            for (uint32_t lane = 0; lane < kTrLanes; ++lane) {
                tr_tally_clear(t[lane]);
                for (uint64_t w = (uint64_t)g * kTrLanes + lane; w < A.ndst; w += stride)
                    tr_copy_word(A, (uint32_t)w, tally, t[lane]);
            }
            if (tally)
                commit_group(A, t.data());
        }
    } else {  // k_transform_transpose
        CHECK(A.tiles == (uint64_t)A.tiles_j * A.tiles_x * (uint64_t)A.sd[A.t] && A.s + A.t == 3 && A.kx + A.kt == 3);
        CHECK(A.axis[0] == A.s && A.axis[A.kx] == 0 && A.axis[A.kt] == A.t);
        std::vector<uint32_t> lin(kTrLdsInWords), lout(kTrLdsOutWords);
        for (uint32_t g = 0; g < groups; ++g) {
            for (uint32_t lane = 0; lane < kTrLanes; ++lane)
                tr_tally_clear(t[lane]);
            for (uint64_t tile = g; tile < A.tiles; tile += groups) {
                const TrTile T = tr_tile(A, (uint32_t)tile);
                CHECK(T.j0 < A.wpd && T.xw0 < A.wps && T.pt >= 0 && T.pt < A.sd[A.t]);
                lin.assign(kTrLdsInWords, 0xDEADBEEFu);
                lout.assign(kTrLdsOutWords, 0xDEADBEEFu);
                std::vector<uint8_t> in_set(kTrLdsInWords, 0), out_set(kTrLdsOutWords, 0);
                for (uint32_t lane = 0; lane < kTrLanes; ++lane)  // load
                    for (uint32_t e = 0; e < kTrLoads; ++e) {
                        uint32_t r, xl;
                        tr_load_slot(lane, e, r, xl);
                        CHECK(r < kTrRows && xl < kTrTX);
                        const uint32_t i = tr_lds_in(r, xl);
                        tr_check(kTrLdsIn, i);
                        in_set[i]++;
                        lin[i] = tr_load_word(A, T, r, xl);
                    }
                for (uint32_t half = 0; half < kTrLanes / 32u; ++half)  // transpose
                    for (uint32_t b = 0; b < kTrBlocks; ++b) {
                        uint32_t jl, xl, v[32];
                        tr_block(half, b, jl, xl);
                        CHECK(jl < kTrTJ && xl < kTrTX);
                        for (uint32_t i = 0; i < 32u; ++i) {
                            const uint32_t a = tr_lds_in(32u * jl + i, xl);
                            tr_check(kTrLdsIn, a);
                            CHECK(in_set[a] == 1);
                            v[i] = lin[a];
                        }
                        butterfly(v);
                        for (uint32_t i = 0; i < 32u; ++i) {
                            const uint32_t a = tr_lds_out(32u * xl + i, jl);
                            tr_check(kTrLdsOut, a);
                            out_set[a]++;
                            lout[a] = tr_finish_word(A, v[i]);
                        }
                    }
                for (uint32_t lane = 0; lane < kTrLanes; ++lane)  // store
                    for (uint32_t e = 0; e < kTrLoads; ++e) {
                        uint32_t xrow, jl;
                        tr_store_slot(lane, e, xrow, jl);
                        CHECK(xrow < kTrXRows && jl < kTrTJ);
                        const uint32_t a = tr_lds_out(xrow, jl);
                        tr_check(kTrLdsOut, a);
                        CHECK(out_set[a] == 1);
                        tr_store_word(A, T, xrow, jl, lout[a], tally, t[lane]);
                    }
            }
            if (tally)
                commit_group(A, t.data());
        }
    }
    for (uint64_t i = 0; i < A.ndst; ++i)
        CHECK(g_stores[i] == 1);  // every destination word has exactly one store
    for (uint32_t i = 0; i < 4u; ++i)
        CHECK(dst[A.ndst + i] == guard && summary[kTrSumWords + i] == guard);
    if (!tally)
        for (uint32_t i = 0; i < kTrSumWords; ++i) {
            CHECK(summary[i] == guard);
            summary[i] = 0u;
        }

    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    fwrite(summary.data(), 4, kTrSumWords, out);
    fwrite(dst.data(), 4, A.ndst, out);
    fclose(out);
    printf("%llu words, %u workgroups, %llu indices checked, failures %d\n%s\n", (unsigned long long)A.ndst, groups,
           (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
