// vxrt_rule.hip -- neighbour-count voxel rules over a box of the resident brickmap (include/vxrt.h, vxrt_apply_rule; host side
// in vxrt_api_query.hip, the shared logic in vxrt_rule.hpp).  A call is these launches on the caller's stream, their number
// fixed by the arguments alone (no host synchronisation):
//
//   k_read_region  (vxrt_region.hip, unchanged) the halo's solid bits into the W_0 plane.
//   k_rule_setup   one lane per plane word: the voxels outside the world ORed into W_0 when `outside` is 1, the F plane built
//                  (the mask funnel-shifted to its bit offset in the halo's words); the first lanes initialise the summary.
//   k_rule_round   `iterations` launches, one lane per plane word, lanes along the words of a row: the nine rows around the
//                  word (27 loads of words the neighbouring lanes and waves load too: L1 / L2 hits) summed to the bit-sliced
//                  count, the two tables looked up through mux trees, the new word stored into the other of two planes.
//                  The neighbourhood is a template parameter, the tables are kernel arguments.
//   k_rule_output  one lane per word of d_bits, grid-stride: W_n, W_n-1 and W_0 funnel-shifted out of the halo's words, cut
//                  to the world voxels of B; W_n stored; the counts and the changed box summed per lane, then per wave, then
//                  per workgroup; one atomic per counter and workgroup.
#include <cstddef>

#include "../../include/vxrt.h"
#include "vxrt_rule.hpp"

namespace vxrt {

static_assert(sizeof(vxrt_rule_summary) == 4u * kRuleSumWords, "rule summary layout");
static_assert(offsetof(vxrt_rule_summary, changed_last) == 4u * kRuleSumLast, "rule summary layout");
static_assert(offsetof(vxrt_rule_summary, changed_min) == 4u * kRuleSumMin, "rule summary layout");
static_assert(offsetof(vxrt_rule_summary, changed_max) == 4u * kRuleSumMax, "rule summary layout");
static_assert(sizeof(vxrt_rule) == 32, "rule layout");
static_assert(VXRT_RULE_MAX_ITERATIONS == kRuleMaxIterations, "rule limits");
static_assert(VXRT_RULE_N6 == kRuleN6 && VXRT_RULE_N18 == kRuleN18 && VXRT_RULE_N26 == kRuleN26, "rule neighbourhoods");
static_assert(VXRT_RULE_BOX == kRuleBox && VXRT_RULE_WORLD == kRuleWorld, "rule scopes");

__global__ __launch_bounds__(256) void k_rule_setup(const RuleArgs A)
{
    const uint64_t i = flat_thread();
    if (i < kRuleSumWords)
        A.summary[i] = rule_summary_init((uint32_t)i);
    if (i < A.np)
        rule_setup_lane(A, i);
}

template <int NB>
__global__ __launch_bounds__(256) void k_rule_round(const RuleArgs A, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst)
{
    const uint64_t i = flat_thread();
    if (i < A.np)
        rule_round_lane<NB>(A, src, dst, i);
}

__global__ __launch_bounds__(256) void k_rule_output(const RuleArgs A, const uint32_t* __restrict__ last, const uint32_t* __restrict__ prev)
{
    __shared__ uint32_t part[4][11];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    RuleTally t;
    rule_tally_clear(t);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < A.nb; i += (uint64_t)gridDim.x * 256u)
        rule_output_lane(A, last, prev, i, t);
#pragma unroll
    for (uint32_t k = 0; k < 5u; ++k) {
        const uint32_t v = wave_sum(t.n[k]);
        if (lane == 0u)
            part[wave][k] = v;
    }
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        const int32_t lo = wave_min(t.lo[k]), hi = wave_max(t.hi[k]);
        if (lane == 0u) {
            part[wave][5u + k] = (uint32_t)lo;
            part[wave][8u + k] = (uint32_t)hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 11u) {
        const uint32_t k = threadIdx.x;
        if (k < 5u) {
            const uint32_t v = part[0][k] + part[1][k] + part[2][k] + part[3][k];
            if (v)
                atomicAdd(A.summary + k, v);
        } else {
            int32_t v = (int32_t)part[0][k];
            for (uint32_t w = 1; w < 4u; ++w) {
                const int32_t o = (int32_t)part[w][k];
                v = k < 8u ? (o < v ? o : v) : (o > v ? o : v);
            }
            int32_t* box = (int32_t*)A.summary;
            if (k < 8u) {
                if (v != INT32_MAX)
                    atomicMin(box + kRuleSumMin + (k - 5u), v);
            } else if (v != INT32_MIN) {
                atomicMax(box + kRuleSumMax + (k - 8u), v);
            }
        }
    }
}

template <int NB>
static void rule_round_launch(const RuleArgs& A, int32_t i, hipStream_t stream)
{
    hipLaunchKernelGGL(k_rule_round<NB>, grid_2d((A.np + 255u) / 256u), dim3(256), 0, stream, A, rule_src(A, i), rule_dst(A, i));
}

// host entry point (vxrt_api_query.hip): arguments validated there (rule_check and rule_layout accept them).  Asynchronous
// on `stream`.
hipError_t apply_rule(const CollideWorld& W, const int32_t o[3], const int32_t d[3], const vxrt_rule& rule, const uint32_t* mask,
                      void* work, uint32_t* bits, vxrt_rule_summary* summary, hipStream_t stream)
{
    RuleLayout L;
    if (rule_check(rule) != 0 || !rule_layout(o, d, rule_halo(rule), L))
        return hipErrorInvalidValue;
    RuleArgs A{};
    rule_args(A, L, W, o, d, rule, mask, work, bits, (uint32_t*)summary);
    hipError_t e;
    if ((e = read_region(W, L.ho, L.hd, A.w0, stream)) != hipSuccess)
        return e;
    const dim3 wg(256);
    hipLaunchKernelGGL(k_rule_setup, grid_2d((L.np + 255u) / 256u), wg, 0, stream, A);
    for (int32_t i = 0; i < rule.iterations; ++i) {
        if (rule.neighbours == kRuleN6)
            rule_round_launch<kRuleN6>(A, i, stream);
        else if (rule.neighbours == kRuleN18)
            rule_round_launch<kRuleN18>(A, i, stream);
        else
            rule_round_launch<kRuleN26>(A, i, stream);
    }
    // few workgroups, each lane taking several words in turn: every workgroup ends in up to 11 atomics on the same 11 words,
    // and with one workgroup per 256 words those atomics, not the words, were the kernel's time (as in k_light_tally)
    const uint64_t tb = (L.nb + 255u) / 256u, few = tb / 8u < 128u ? (tb < 128u ? tb : 128u) : tb / 8u;
    hipLaunchKernelGGL(k_rule_output, dim3((unsigned)(few < 1024u ? few : 1024u)), wg, 0, stream, A, rule_src(A, rule.iterations),
                       rule_src(A, rule.iterations - 1));
    return hipGetLastError();
}

}  // namespace vxrt
