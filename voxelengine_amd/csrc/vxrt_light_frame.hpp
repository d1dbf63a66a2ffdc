// vxrt_light_frame.hpp -- light on frames (include/vxrt.h, vxrt_light_frame): the per-pixel logic shared by the kernel of
// vxrt_light_frame.hip, the host side in vxrt_api_query.hip and the host harnesses of the tests (tests/tools/
// lightframe_check.cpp and lightframe_args_check.cpp, through tests/tools/hoststub): the checks of the parameters, the voxel
// face a pixel shows, the nine cells in front of it with their solidity and light levels, the four corner triples
// (sky, block, occlusion), the position of the pixel on the face, the interpolation, the colour and the stores.
//
// The frame and the shared helpers are vxrt_frame.hpp's, the launch is the temporal filter's (rp_launch_shape,
// rp_wave_pixel).  A pixel reads its own colour, key and hit index, the cell records and brick words of nine voxels and up to nine level bytes, and writes its own colour, terms and BGRA8 pixel.
// The work splits in three: lf_load reads the pixel's own inputs and names its voxel face, lf_face makes the four corner
// triples of a face from the world and the levels alone, lf_shade places the pixel on its face and relights it.
#pragma once

#include "vxrt_region.hpp"     // CollideWorld
#include "vxrt_reproject.hpp"  // the launch shape (and with it vxrt_frame.hpp)

// The harness defines this to check every index the code forms into an input, an output, the world tables or the level
// bytes against that array's size (array: one of the kLf* ids below).  The kernel leaves it empty.
#ifndef VXRT_LF_CHECK
#define VXRT_LF_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint32_t kLfSmooth = 1u, kLfOcclusion = 2u;     // VXRT_LF_SMOOTH, VXRT_LF_OCCLUSION
constexpr uint64_t kLfMaxBoxVoxels = 1ull << 28;          // vxrt_light_field's limit on dims[0] * dims[1] * dims[2]
enum { kLfColorIn, kLfKeys, kLfHit, kLfLevels, kLfColorOut, kLfFb, kLfTerms, kLfMeta, kLfPool, kLfArrays };
// what became of a pixel: the counters of vxrt_light_frame_summary it adds to (a miss: none)
enum { kLfHitBit = 1u, kLfInBoxBit = 2u, kLfOccludedBit = 4u, kLfDarkBit = 8u };

// what the launch reads and writes (device pointers; host pointers in the harness)
struct LightFrameArgs {
    const float* color_in;   // W * H * 3
    const uint32_t* keys;    // W * H
    const long long* hit;    // W * H
    const uint8_t* levels;   // bd[0] * bd[1] * bd[2] bytes in region order, or NULL
    float* color_out;        // W * H * 3
    uint32_t* fb;            // W * H BGRA8 pixels, or NULL
    float* terms;            // W * H * 3, or NULL
    uint32_t* summary;       // hit, in_box, occluded, dark, or NULL
    uint32_t W, H;
    uint32_t flags, outside_level;
    float sky_floor, block_color[3], ao_curve[4];
    int32_t bo[3], bd[3];    // the light box
};

// The parameter checks of include/vxrt.h that need neither the context nor a pointer of the call: 0 when all pass, else
// the place of the first that fails in the documented order (2: W or H; 3: params or its struct_size; 4: flags,
// outside_level or reserved_; 5: sky_floor; 6: block_color or ao_curve; 7: the pose; 8: the box).
inline int light_frame_check(uint32_t W, uint32_t H, const vxrt_light_frame_params* p)
{
    if (!denoise_frame_ok(W, H))
        return 2;
    if (!p || p->struct_size != sizeof(vxrt_light_frame_params))
        return 3;
    if ((p->flags & ~(kLfSmooth | kLfOcclusion)) != 0u || p->outside_level > 0xFFu || p->reserved_ != 0)
        return 4;
    if (!(p->sky_floor >= 0.0f && p->sky_floor <= 1.0f))  // (a NaN fails)
        return 5;
    for (int k = 0; k < 3; ++k)
        if (!(p->block_color[k] >= 0.0f) || !frame_finite(p->block_color[k]))
            return 6;
    for (int k = 0; k < 4; ++k)
        if (!(p->ao_curve[k] >= 0.0f) || !frame_finite(p->ao_curve[k]))
            return 6;
    if (!pose_finite(p->cam))
        return 7;
    uint64_t voxels = 1u;
    for (int k = 0; k < 3; ++k) {
        if (p->box_dims[k] < 1 || (int64_t)p->box_origin[k] + p->box_dims[k] > INT32_MAX)
            return 8;
        voxels *= (uint64_t)p->box_dims[k];  // (each factor below 2^31, checked against 2^28 before the next: no overflow)
        if (voxels > kLfMaxBoxVoxels)
            return 8;
    }
    return 0;
}

// the call's arguments as the launch takes them (params checked before)
inline void light_frame_args(LightFrameArgs& A, uint32_t W, uint32_t H, const vxrt_light_frame_params& p)
{
    A.W = W;
    A.H = H;
    A.flags = p.flags;
    A.outside_level = p.outside_level;
    A.sky_floor = p.sky_floor;
    for (int k = 0; k < 3; ++k) {
        A.block_color[k] = p.block_color[k];
        A.bo[k] = p.box_origin[k];
        A.bd[k] = p.box_dims[k];
    }
    for (int k = 0; k < 4; ++k)
        A.ao_curve[k] = p.ao_curve[k];
}

// whether voxel (x, y, z) is solid: one cell record and, for a cell that holds a brick, one brick word; empty outside the world
__host__ __device__ inline bool lf_solid(const CollideWorld& Wd, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x >= Wd.dim[0] || y >= Wd.dim[1] || z >= Wd.dim[2])
        return false;
    const uint64_t cell = hbm_index(x >> Wd.lgf, y >> Wd.lgf, z >> Wd.lgf, Wd.cx, Wd.cz);
    VXRT_LF_CHECK(kLfMeta, cell);
    const uint32_t slot = Wd.meta[cell].x;
    if (slot == kEmptySlot)
        return false;
    const uint32_t m = (uint32_t)Wd.f - 1u, f = (uint32_t)Wd.f;
    const uint32_t bit = ((uint32_t)x & m) + f * (((uint32_t)z & m) + f * ((uint32_t)y & m));  // (HBM order inside a brick)
    const uint64_t word = (uint64_t)slot * ((f * f * f) >> 5) + (bit >> 5);
    VXRT_LF_CHECK(kLfPool, word);
    return (Wd.pool[word] >> (bit & 31u)) & 1u;
}

// lev(q) of an EMPTY cell q: its byte of the levels when it lies in the box and the levels are given, else outside_level
__host__ __device__ inline uint32_t lf_level(const LightFrameArgs& A, int x, int y, int z, bool& in_box)
{
    // (q in -1 .. 2^24 and an int32 origin: the difference needs 64 bits)
    const int64_t r0 = (int64_t)x - A.bo[0], r1 = (int64_t)y - A.bo[1], r2 = (int64_t)z - A.bo[2];
    in_box = A.levels != nullptr && r0 >= 0 && r1 >= 0 && r2 >= 0 && r0 < A.bd[0] && r1 < A.bd[1] && r2 < A.bd[2];
    if (!in_box)
        return A.outside_level;
    const uint32_t at = (uint32_t)r0 + (uint32_t)A.bd[0] * ((uint32_t)r1 + (uint32_t)A.bd[1] * (uint32_t)r2);  // < 2^28
    VXRT_LF_CHECK(kLfLevels, at);
    return A.levels[at];
}

// the four corners of a face, corner (i, j) at index i + 2 * j: LS, LB and A of the contract, and the face's kLf* bits
// (in_box, occluded)
struct LfFace {
    float ls[4], lb[4], ao[4];
    uint32_t bits;
};

// The face of voxel v on axis a (0 .. 2) seen from the side `toward` names.  The nine solidity lookups and the nine level
// loads are unconditional but for the world's and the box's bounds, so that they are in flight together.
__host__ __device__ inline LfFace lf_face(const LightFrameArgs& A, const CollideWorld& Wd, const int32_t v[3], uint32_t a, bool toward)
{
    const int step = toward ? -1 : 1;
    const int f[3] = {v[0] + (a == 0u ? step : 0), v[1] + (a == 1u ? step : 0), v[2] + (a >= 2u ? step : 0)};
    // e_b and e_c: (b, c) = (1, 2), (0, 2), (0, 1) for a = 0, 1, 2
    const int eb[3] = {a == 0u ? 0 : 1, a == 0u ? 1 : 0, 0}, ec[3] = {0, a >= 2u ? 1 : 0, a >= 2u ? 0 : 1};
    bool s[3][3];
    uint32_t lev[3][3];
    bool front_in_box = false;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int q[3] = {f[0] + i * eb[0] + j * ec[0], f[1] + i * eb[1] + j * ec[1], f[2] + i * eb[2] + j * ec[2]};
            bool in_box;
            const uint32_t l = lf_level(A, q[0], q[1], q[2], in_box);
            s[i + 1][j + 1] = lf_solid(Wd, q[0], q[1], q[2]);
            lev[i + 1][j + 1] = s[i + 1][j + 1] ? 0u : l;
            if (i == 0 && j == 0)
                front_in_box = in_box;
        }
    }
    LfFace F;
    bool occluded = false;
    const uint32_t l00 = lev[1][1];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int si = 2 * i, sj = 2 * j;  // (the corner's neighbours at [si][1], [1][sj] and [si][sj] of the 3 x 3)
            const bool s1 = s[si][1], s2 = s[1][sj], s3 = s[si][sj];
            const bool m1 = !s1, m2 = !s2, m3 = !(s3 || (s1 && s2));
            const uint32_t l1 = m1 ? lev[si][1] : 0u, l2 = m2 ? lev[1][sj] : 0u, l3 = m3 ? lev[si][sj] : 0u;
            const uint32_t cnt = 1u + (m1 ? 1u : 0u) + (m2 ? 1u : 0u) + (m3 ? 1u : 0u);
            const uint32_t sky = (l00 >> 4) + (l1 >> 4) + (l2 >> 4) + (l3 >> 4);
            const uint32_t blk = (l00 & 15u) + (l1 & 15u) + (l2 & 15u) + (l3 & 15u);
            const uint32_t open = (s1 && s2) ? 0u : 3u - ((s1 ? 1u : 0u) + (s2 ? 1u : 0u) + (s3 ? 1u : 0u));
            occluded = occluded || open < 3u;
            const int c = i + 2 * j;
            const bool smooth = (A.flags & kLfSmooth) != 0u;
            F.ls[c] = smooth ? (float)sky / (float)cnt : (float)(l00 >> 4);
            F.lb[c] = smooth ? (float)blk / (float)cnt : (float)(l00 & 15u);
            // (selects: the curve stays in scalar registers)
            const float curve = open == 0u ? A.ao_curve[0] : open == 1u ? A.ao_curve[1] : open == 2u ? A.ao_curve[2] : A.ao_curve[3];
            F.ao[c] = (A.flags & kLfOcclusion) != 0u ? curve : 1.0f;
        }
    }
    F.bits = (front_in_box ? (uint32_t)kLfInBoxBit : 0u) | (occluded ? (uint32_t)kLfOccludedBit : 0u);
    return F;
}

__host__ __device__ inline float lf_bilinear(const float q[4], float u, float w)
{
    const float q0 = q[0] + u * (q[1] - q[0]), q1 = q[2] + u * (q[3] - q[2]);
    return q0 + w * (q1 - q0);
}

// The pixel's own inputs: colour, key and hit index, and what they name.  hit: a hit pixel (else v, a and toward are unset).
struct LfPixel {
    float c[3];
    uint32_t key;
    long long hit_index;
    int32_t v[3];
    uint32_t a;
    float pl;  // the plane of the face
    bool toward, hit;
};

// (Args: what a frame stage's launch reads -- color_in, keys, hit and W; vxrt_material.hpp's stage loads its pixels here too)
template <class Args>
__host__ __device__ inline LfPixel lf_load(const Args& A, const CollideWorld& Wd, uint32_t x, uint32_t y)
{
    const uint32_t i = y * A.W + x;  // W * H <= 2^26: every index fits 32 bits
    VXRT_LF_CHECK(kLfColorIn, 3u * i + 2u);
    VXRT_LF_CHECK(kLfKeys, i);
    VXRT_LF_CHECK(kLfHit, i);
    LfPixel P;
    P.c[0] = A.color_in[3u * i];
    P.c[1] = A.color_in[3u * i + 1u];
    P.c[2] = A.color_in[3u * i + 2u];
    P.key = A.keys[i];
    P.hit_index = A.hit[i];
    P.v[0] = P.v[1] = P.v[2] = 0;
    const FrameFace face = frame_face(P.key);
    P.a = face.a;
    P.pl = face.pl;
    P.toward = face.toward;
    P.hit = false;
    if (P.key == 0u || P.hit_index < 0)
        return P;
    // (as guide_key: X * Y fits 48 bits, X * Y * Z need not fit 64)
    const uint64_t xy = (uint64_t)Wd.dim[0] * (uint64_t)Wd.dim[1], z = (uint64_t)P.hit_index / xy, r = (uint64_t)P.hit_index % xy;
    if (z >= (uint64_t)Wd.dim[2])
        return P;
    P.v[0] = (int32_t)(r % (uint64_t)Wd.dim[0]);
    P.v[1] = (int32_t)(r / (uint64_t)Wd.dim[0]);
    P.v[2] = (int32_t)z;
    P.hit = true;
    return P;
}

// The position (u, w) of hit pixel P on its face, on the axes (b, c), under the primary ray (o, d): clamped to 0 .. 1, the
// centre of the face where the ray does not give one
__host__ __device__ inline void lf_position(const LfPixel& P, const float o[3], const float d[3], float& u, float& w)
{
    const uint32_t a = P.a;
    // (selects, not indexing: the vectors stay in registers)
    const float ob = a == 0u ? o[1] : o[0], db = a == 0u ? d[1] : d[0], oc = a >= 2u ? o[1] : o[2], dc = a >= 2u ? d[1] : d[2];
    const float vb = (float)(a == 0u ? P.v[1] : P.v[0]), vc = (float)(a >= 2u ? P.v[1] : P.v[2]);
    float da;
    const float t = frame_plane_t(a, P.pl, o, d, da);
    u = frame_clamp01((ob + t * db) - vb);
    w = frame_clamp01((oc + t * dc) - vc);
    if (da == 0.0f || !frame_finite(t) || !frame_finite(u) || !frame_finite(w))
        u = w = 0.5f;
}

// Pixel (x, y), loaded into P, with primary ray (o, d) and the corners F of its face (a miss: F is not looked at): its
// colour, terms and BGRA8 pixel stored; returns the kLf* bits of the counters it adds to.
__host__ __device__ inline uint32_t lf_shade(const LightFrameArgs& A, uint32_t x, uint32_t y, const LfPixel& P, const LfFace& F,
                                             const float o[3], const float d[3])
{
    const uint32_t i = y * A.W + x;
    float out[3] = {P.c[0], P.c[1], P.c[2]}, term[3] = {0.0f, 0.0f, 0.0f};
    uint32_t bits = 0u;
    if (P.hit) {
        float u, w;
        lf_position(P, o, d, u, w);
        const float S = lf_bilinear(F.ls, u, w) / 15.0f, Bk = lf_bilinear(F.lb, u, w) / 15.0f, Ao = lf_bilinear(F.ao, u, w);
        const float ks = A.sky_floor + (1.0f - A.sky_floor) * S;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            out[ch] = (P.c[ch] * ks + A.block_color[ch] * Bk) * Ao;
        term[0] = S;
        term[1] = Bk;
        term[2] = Ao;
        bits = kLfHitBit | F.bits | (S == 0.0f && Bk == 0.0f ? (uint32_t)kLfDarkBit : 0u);
    }
    VXRT_LF_CHECK(kLfColorOut, 3u * i + 2u);
    frame_store_color(A.color_out, i, out);
    if (A.fb) {
        VXRT_LF_CHECK(kLfFb, i);
        A.fb[i] = dn_bgra8(out[0], out[1], out[2]);
    }
    if (A.terms) {
        VXRT_LF_CHECK(kLfTerms, 3u * i + 2u);
        A.terms[3u * i] = term[0];
        A.terms[3u * i + 1u] = term[1];
        A.terms[3u * i + 2u] = term[2];
    }
    return bits;
}

// pixel (x, y) with primary ray (o, d), whole
__host__ __device__ inline uint32_t lf_pixel(const LightFrameArgs& A, const CollideWorld& Wd, uint32_t x, uint32_t y, const float o[3],
                                             const float d[3])
{
    const LfPixel P = lf_load(A, Wd, x, y);
    LfFace F{};
    if (P.hit)
        F = lf_face(A, Wd, P.v, P.a, P.toward);
    return lf_shade(A, x, y, P, F, o, d);
}

#ifndef VXRT_HOST_CHECK  // the kernel of vxrt_light_frame.hip
struct RenderArgs;  // (vxrt_kernels.hpp)
// R carries the camera (camera_args, ortho, origin, fwd, up, right), A the rest; cus: the device's compute units
hipError_t light_frame(const RenderArgs& R, const LightFrameArgs& A, const CollideWorld& Wd, uint32_t cus, hipStream_t stream);
#endif

}  // namespace vxrt
