// vxrt_material.hpp -- voxel materials (include/vxrt.h, vxrt_material_field / vxrt_material_frame): the definition of a
// voxel's material and the per-lane and per-pixel logic shared by the kernels of vxrt_material.hip, the host side in
// vxrt_api_query.hip and the host harnesses of the tests (tests/tools/material_check.cpp and material_args_check.cpp,
// through tests/tools/hoststub): the checks of the rules and the parameters, the band and the rule of a voxel, the paint
// lookup, the task cut of a field launch, the march of a field lane down y, and a frame pixel's material, texel and colour.
//
// Field.  A lane owns four x-consecutive voxels of one z of the box (so that its bytes are one dword where the row length
// and the output's address allow) and marches down the rows of one y segment, carrying run -- the solid voxels directly
// above, capped at 16 -- in a register per voxel: run(y) = solid(y + 1) ? min(run(y + 1) + 1, 16) : 0.  It starts 16 rows
// above its segment with run 0: after 16 rows the capped run is exact whatever lies higher.  Solidity is the region layer's
// row word (region_row_word), one word per 32 voxels and row, which the eight lanes of those voxels load together.
// Frame.  The pixel's own inputs, its voxel face and its position on the face are vxrt_light_frame.hpp's (lf_load,
// lf_position); the run of the hit voxel is a walk of at most under_depth + 1 voxels up its column (lf_solid).
#pragma once

#include "vxrt_light_frame.hpp"  // lf_load, lf_position, lf_solid (and with it vxrt_frame.hpp and vxrt_region.hpp)

// The harness defines this to check every index the code forms into the paint, the palette, the atlas, an output or the
// tally against that array's size (array: one of the kMat* ids below; the frame's inputs and the world tables are checked
// under VXRT_LF_CHECK with the kLf* ids).  The kernels leave it empty.
#ifndef VXRT_MAT_CHECK
#define VXRT_MAT_CHECK(array, index)
#endif

namespace vxrt {

constexpr uint32_t kMatRunCap = 16u;       // a run is carried up to here: under_depth <= 15 never asks for more
constexpr uint32_t kMatMaxTiles = 4096u, kMatMaxTileShift = 6u;
constexpr uint32_t kMatTallyWords = 260u;  // vxrt_material_summary as words: solid, painted, top, reserved, hist[256]
constexpr uint32_t kMatSegment = 64u, kMatMinSegment = 16u;  // rows of a y segment of a field launch
enum { kMatPaint = kLfArrays, kMatOut, kMatTally, kMatPalette, kMatAtlas, kMatAov, kMatArrays };
// what became of a frame pixel: the counters of vxrt_material_frame_summary it adds to (a miss: none)
enum { kMatHitBit = 1u, kMatPaintedBit = 2u, kMatTopBit = 4u, kMatTexturedBit = 8u };

// ---- the rules -------------------------------------------------------------------------------------------------------
// 0 when the rules pass, else the place of the first check that fails in the documented order (1: NULL or struct_size;
// 2: n_bands; 3: a band; 4: reserved_).  The paint box is material_paint_ok's: it is looked at only with paint.
inline int material_rules_check(const vxrt_material_rules* r)
{
    if (!r || r->struct_size != sizeof(vxrt_material_rules))
        return 1;
    if (r->n_bands < 1u || r->n_bands > (uint32_t)VXRT_MATERIAL_MAX_BANDS)
        return 2;
    for (uint32_t i = 0; i < r->n_bands; ++i) {
        const vxrt_material_band& b = r->bands[i];
        if (i == 0u ? b.y_from != INT32_MIN : b.y_from <= r->bands[i - 1u].y_from)
            return 3;
        if (b.top == 0u || b.under == 0u || b.deep == 0u || b.under_depth > 15u)
            return 3;
    }
    return r->reserved_ != 0 ? 4 : 0;
}

// the paint box within the limits of vxrt_light_frame's box
inline bool material_paint_ok(const vxrt_material_rules& r)
{
    uint64_t voxels = 1u;
    for (int k = 0; k < 3; ++k) {
        if (r.paint_dims[k] < 1 || (int64_t)r.paint_origin[k] + r.paint_dims[k] > INT32_MAX)
            return false;
        voxels *= (uint64_t)r.paint_dims[k];  // (each factor below 2^31, checked against 2^28 before the next: no overflow)
        if (voxels > kLfMaxBoxVoxels)
            return false;
    }
    return true;
}

// the band of altitude y as one word: top | under << 8 | deep << 16 | under_depth << 24 (selects over the bands in use: the
// rules are kernel arguments and stay in scalar registers)
__host__ __device__ inline uint32_t mat_band(const vxrt_material_rules& R, int32_t y)
{
    uint32_t w = 0u;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)VXRT_MATERIAL_MAX_BANDS; ++i) {
        const vxrt_material_band& b = R.bands[i];
        const uint32_t bw = (uint32_t)b.top | (uint32_t)b.under << 8 | (uint32_t)b.deep << 16 | (uint32_t)b.under_depth << 24;
        w = i < R.n_bands && b.y_from <= y ? bw : w;  // (bands[0].y_from is INT32_MIN: some band always holds y)
    }
    return w;
}

// rule(v) of a voxel in band word `band` with `run` solid voxels above it (run may be capped anywhere above under_depth)
__host__ __device__ inline uint32_t mat_rule(uint32_t band, uint32_t run)
{
    return run == 0u ? band & 0xFFu : run <= band >> 24 ? (band >> 8) & 0xFFu : (band >> 16) & 0xFFu;
}

// the paint byte of voxel (x, y, z): 0 without paint, outside P, or where the byte is 0
__host__ __device__ inline uint32_t mat_paint(const vxrt_material_rules& R, const uint8_t* paint, int64_t x, int64_t y, int64_t z)
{
    const int64_t r0 = x - R.paint_origin[0], r1 = y - R.paint_origin[1], r2 = z - R.paint_origin[2];
    if (paint == nullptr || r0 < 0 || r1 < 0 || r2 < 0 || r0 >= R.paint_dims[0] || r1 >= R.paint_dims[1] || r2 >= R.paint_dims[2])
        return 0u;
    const uint32_t at = (uint32_t)r0 + (uint32_t)R.paint_dims[0] * ((uint32_t)r1 + (uint32_t)R.paint_dims[1] * (uint32_t)r2);  // < 2^28
    VXRT_MAT_CHECK(kMatPaint, at);
    return paint[at];
}

// ---- the field -------------------------------------------------------------------------------------------------------
// what the launch reads and writes (device pointers; host pointers in the harness)
struct MaterialFieldArgs {
    vxrt_material_rules rules;
    const uint8_t* paint;  // paint_dims[0] * [1] * [2] bytes in region order, or NULL
    uint8_t* out;          // d[0] * d[1] * d[2] bytes in region order
    uint32_t* summary;     // kMatTallyWords words
    int32_t o[3], d[3];
    // the task cut: a task is one wave; a row takes L = 1 << lgL lanes of four voxels (all 64 lanes, nxc chunks of 256
    // voxels, for rows longer than 252), a wave 64 / L consecutive z, a task `seg` consecutive rows
    uint32_t seg, lgL, nxc, nys, nzg;
    uint32_t dword;        // rows and output address allow one dword store per lane and row
    uint64_t tasks;
};

// The limits of a field's box: 0 when they hold, 1 for the dims (1 <= dims[k], their product <= 2^28), 2 for the origin
// (origin[k] + dims[k] + 16 <= 2^31 - 1: the warm-up rows above the box have int32 coordinates).
inline int material_box_check(const int32_t o[3], const int32_t d[3])
{
    if (box_voxels(d, kLfMaxBoxVoxels) == 0)
        return 1;
    for (int k = 0; k < 3; ++k)
        if ((int64_t)o[k] + d[k] + (int64_t)kMatRunCap > INT32_MAX)
            return 2;
    return 0;
}

// the launch's arguments for box (o, d) cut into y segments of `seg` rows (checked before; seg >= 1), bytes to `out`
inline void material_field_args(MaterialFieldArgs& A, const vxrt_material_rules& rules, const int32_t o[3], const int32_t d[3], uint32_t seg,
                                uint8_t* out)
{
    A.rules = rules;
    A.out = out;
    for (int k = 0; k < 3; ++k) {
        A.o[k] = o[k];
        A.d[k] = d[k];
    }
    const uint32_t quads = ((uint32_t)d[0] + 3u) >> 2;
    A.lgL = 0u;
    while (A.lgL < 6u && (1u << A.lgL) < quads)
        ++A.lgL;
    A.nxc = (quads + 63u) >> 6;
    A.seg = seg;
    A.nys = (uint32_t)(((uint64_t)d[1] + seg - 1u) / seg);
    const uint32_t zpw = 64u >> A.lgL;
    A.nzg = ((uint32_t)d[2] + zpw - 1u) / zpw;
    A.tasks = (uint64_t)A.nxc * A.nys * A.nzg;  // at most the box's voxels
    A.dword = (d[0] & 3) == 0 && ((uintptr_t)A.out & 3u) == 0u ? 1u : 0u;
}

// The rows of a y segment for box dims d on a device of `cus` compute units: kMatSegment, halved down to kMatMinSegment while
// the cut gives fewer tasks than eight waves per SIMD.  A lane's march is a chain of dependent loads (cell record, brick
// word) per row, so a small box wants many short tasks in flight, a large one long tasks with little warm-up.
inline uint32_t material_field_segment(const int32_t d[3], uint32_t cus)
{
    uint32_t seg = kMatSegment;
    for (; seg > kMatMinSegment; seg >>= 1) {
        MaterialFieldArgs A{};
        const int32_t o[3] = {0, 0, 0};
        material_field_args(A, vxrt_material_rules{}, o, d, seg, nullptr);
        if (A.tasks >= 32ull * cus)
            break;
    }
    return seg;
}

// the solidity of four voxels x0w + sh .. + 3 of world row (wy, wz) as a nibble; a row outside the world is empty (no load)
__host__ __device__ inline uint32_t mat_row_nibble(const CollideWorld& Wd, bool xz_in, int64_t x0w, uint32_t sh, int64_t wy, int64_t wz)
{
    if (!xz_in || wy < 0 || wy >= Wd.dim[1])
        return 0u;
    VXRT_MAT_CHECK(kLfMeta, hbm_index(Wd.cx - 1, (int)wy >> Wd.lgf, (int)wz >> Wd.lgf, Wd.cx, Wd.cz));  // the row's last cell record
    return (region_row_word(Wd.meta, Wd.pool, Wd.f, Wd.lgf, Wd.cx, Wd.cz, x0w, (int)wy, (int)wz) >> sh) & 15u;
}

// Lane `lane` of task `task`: its four voxels down its y segment, bytes stored, counts added to `tally` (kMatTallyWords
// words shared by the workgroup: LDS in the kernel).  hist[0] is counted with the rest: empty voxels of the box.
__host__ __device__ inline void mat_field_lane(const MaterialFieldArgs& A, const CollideWorld& Wd, uint64_t task, uint32_t lane, uint32_t* tally)
{
    const uint32_t xc = (uint32_t)(task % A.nxc);
    const uint64_t t = task / A.nxc;
    const uint32_t ys = (uint32_t)(t % A.nys), zg = (uint32_t)(t / A.nys);
    const uint32_t L = 1u << A.lgL, dx = (uint32_t)A.d[0], dy = (uint32_t)A.d[1], dz = (uint32_t)A.d[2];
    const uint32_t xl = 4u * (xc * 64u + (lane & (L - 1u))), zl = zg * (64u >> A.lgL) + (lane >> A.lgL);
    if (xl >= dx || zl >= dz)
        return;
    const uint32_t y_lo = ys * A.seg;  // (ys < nys: below dy)
    const uint32_t y_hi = (uint32_t)((uint64_t)y_lo + A.seg < dy ? (uint64_t)y_lo + A.seg : dy) - 1u;
    const int64_t wz = (int64_t)A.o[2] + zl, wx = (int64_t)A.o[0] + xl;
    const int64_t x0w = (int64_t)A.o[0] + 32 * (int64_t)(xl >> 5);
    const uint32_t sh = xl & 31u;
    const bool xz_in = wz >= 0 && wz < Wd.dim[2] && x0w + 31 >= 0 && x0w < Wd.dim[0];
    const uint32_t valid = dx - xl < 4u ? dx - xl : 4u;  // the lane's voxels inside the box
    uint32_t run[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = kMatRunCap; k >= 1u; --k) {  // the warm-up: rows y_hi + 16 .. y_hi + 1
        const uint32_t n = mat_row_nibble(Wd, xz_in, x0w, sh, (int64_t)A.o[1] + y_hi + k, wz);
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
            run[j] = (n >> j) & 1u ? (run[j] < kMatRunCap ? run[j] + 1u : kMatRunCap) : 0u;
    }
    uint32_t n_solid = 0u, n_painted = 0u, n_top = 0u, n_empty = 0u;
    uint32_t last_m = 0u, last_n = 0u;  // a run of equal bytes, counted into hist in one go
    uint32_t at = xl + dx * (y_hi + dy * zl);  // < 2^28
    for (uint32_t y = y_hi + 1u; y-- > y_lo; at -= dx) {
        const int64_t wy = (int64_t)A.o[1] + y;
        const uint32_t n = mat_row_nibble(Wd, xz_in, x0w, sh, wy, wz);
        const uint32_t band = mat_band(A.rules, (int32_t)wy);
        uint32_t bytes = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const bool solid = (n >> j) & 1u;
            if (j < valid) {
                uint32_t m = 0u;
                if (solid) {
                    const uint32_t p = mat_paint(A.rules, A.paint, wx + j, wy, wz);
                    m = p ? p : mat_rule(band, run[j]);
                    ++n_solid;
                    n_painted += p ? 1u : 0u;
                    n_top += run[j] == 0u ? 1u : 0u;
                    if (m != last_m) {
                        if (last_n) {
                            VXRT_MAT_CHECK(kMatTally, 4u + last_m);
                            atom_add(&tally[4u + last_m], last_n);
                        }
                        last_m = m;
                        last_n = 0u;
                    }
                    ++last_n;
                } else {
                    ++n_empty;
                }
                bytes |= m << (8u * j);
            }
            run[j] = solid ? (run[j] < kMatRunCap ? run[j] + 1u : kMatRunCap) : 0u;
        }
        if (A.dword) {  // (dx a multiple of four: all four voxels are in the row, and `at` is one too)
            VXRT_MAT_CHECK(kMatOut, at + 3u);
            *reinterpret_cast<uint32_t*>(A.out + at) = bytes;
        } else {
            for (uint32_t j = 0; j < valid; ++j) {
                VXRT_MAT_CHECK(kMatOut, at + j);
                A.out[at + j] = (uint8_t)(bytes >> (8u * j));
            }
        }
    }
    if (last_n) {
        VXRT_MAT_CHECK(kMatTally, 4u + last_m);
        atom_add(&tally[4u + last_m], last_n);
    }
    VXRT_MAT_CHECK(kMatTally, 4u);
    if (n_solid)
        atom_add(&tally[0], n_solid);
    if (n_painted)
        atom_add(&tally[1], n_painted);
    if (n_top)
        atom_add(&tally[2], n_top);
    if (n_empty)
        atom_add(&tally[4], n_empty);
}

// ---- the frame -------------------------------------------------------------------------------------------------------
// what the launch reads and writes (device pointers; host pointers in the harness)
struct MaterialFrameArgs {
    vxrt_material_rules rules;
    const float* color_in;         // W * H * 3
    const uint32_t* keys;          // W * H
    const long long* hit;          // W * H
    const uint8_t* paint;          // the paint box's bytes, or NULL
    const vxrt_material* palette;  // 256 entries
    const uint32_t* atlas;         // n_tiles * T * T RGBA8 texels, or NULL
    float* color_out;              // W * H * 3
    uint32_t* fb;                  // W * H BGRA8 pixels, or NULL
    uint8_t* aov;                  // W * H material ids, or NULL
    uint32_t* summary;             // hit, painted, top, textured, or NULL
    uint32_t W, H;
    uint32_t n_tiles, tile_shift;
};

// The parameter checks of include/vxrt.h that need neither the context nor a buffer of the call: 0 when all pass, else the
// place of the first that fails in the documented order (2: W or H; 3: params or its struct_size; 4: n_tiles, tile_shift or
// reserved_; 5 .. 8: the rules (material_rules_check + 4); 9: the pose; 10: the paint box, looked at only with paint).
inline int material_frame_check(uint32_t W, uint32_t H, const vxrt_material_frame_params* p, const vxrt_material_rules* rules, bool paint)
{
    if (!denoise_frame_ok(W, H))
        return 2;
    if (!p || p->struct_size != sizeof(vxrt_material_frame_params))
        return 3;
    if (p->n_tiles > kMatMaxTiles || p->tile_shift > kMatMaxTileShift || p->reserved_ != 0)
        return 4;
    if (const int r = material_rules_check(rules))
        return 4 + r;
    if (!pose_finite(p->cam))
        return 9;
    return paint && !material_paint_ok(*rules) ? 10 : 0;
}

// Pixel (x, y) with primary ray (o, d): its colour, BGRA8 pixel and material id stored; returns the kMat* bits of the
// counters it adds to.
__host__ __device__ inline uint32_t mat_pixel(const MaterialFrameArgs& A, const CollideWorld& Wd, uint32_t x, uint32_t y, const float o[3],
                                              const float d[3])
{
    const uint32_t i = y * A.W + x;  // W * H <= 2^26: every index fits 32 bits
    const LfPixel P = lf_load(A, Wd, x, y);
    float out[3] = {P.c[0], P.c[1], P.c[2]};
    uint32_t bits = 0u, m = 0u;
    if (P.hit) {
        const uint32_t band = mat_band(A.rules, P.v[1]), depth = band >> 24;
        uint32_t run = 0u;  // (at most depth + 1 voxels looked at: run == depth + 1 stands for every longer run)
        while (run <= depth && lf_solid(Wd, P.v[0], P.v[1] + (int)run + 1, P.v[2]))
            ++run;
        const uint32_t p = mat_paint(A.rules, A.paint, P.v[0], P.v[1], P.v[2]);
        m = p ? p : mat_rule(band, run);
        bits = kMatHitBit | (p ? (uint32_t)kMatPaintedBit : 0u) | (run == 0u ? (uint32_t)kMatTopBit : 0u);
        float u, w;
        lf_position(P, o, d, u, w);
        VXRT_MAT_CHECK(kMatPalette, m);
        const vxrt_material e = A.palette[m];
        const uint32_t tile = P.a != 1u ? e.tile_side : P.toward ? e.tile_bottom : e.tile_top;
        float tex[3] = {1.0f, 1.0f, 1.0f};
        if (A.atlas != nullptr && tile < A.n_tiles) {
            const int T = 1 << A.tile_shift;
            int iu = (int)(u * (float)T), iw = (int)(w * (float)T);
            iu = iu < T - 1 ? iu : T - 1;
            iw = iw < T - 1 ? iw : T - 1;
            const int s = P.a == 0u ? iw : iu, r = P.a == 0u ? T - 1 - iu : P.a == 1u ? iw : T - 1 - iw;
            const uint32_t at = (((tile << A.tile_shift) + (uint32_t)r) << A.tile_shift) + (uint32_t)s;  // < 2^12 * 2^6 * 2^6
            VXRT_MAT_CHECK(kMatAtlas, at);
            const uint32_t texel = A.atlas[at];
            tex[0] = (float)(texel & 0xFFu) / 255.0f;
            tex[1] = (float)((texel >> 8) & 0xFFu) / 255.0f;
            tex[2] = (float)((texel >> 16) & 0xFFu) / 255.0f;
            bits |= kMatTexturedBit;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float alb = e.tint[ch] * tex[ch];
            out[ch] = P.c[ch] * alb;
        }
    }
    VXRT_MAT_CHECK(kLfColorOut, 3u * i + 2u);
    frame_store_color(A.color_out, i, out);
    if (A.fb) {
        VXRT_MAT_CHECK(kLfFb, i);
        A.fb[i] = dn_bgra8(out[0], out[1], out[2]);
    }
    if (A.aov) {
        VXRT_MAT_CHECK(kMatAov, i);
        A.aov[i] = (uint8_t)m;
    }
    return bits;
}

#ifndef VXRT_HOST_CHECK  // the kernels of vxrt_material.hip
struct RenderArgs;  // (vxrt_kernels.hpp)
// A.summary and A.paint set, the rest by material_field_args
hipError_t material_field(const MaterialFieldArgs& A, const CollideWorld& Wd, hipStream_t stream);
// R carries the camera (camera_args, ortho, origin, fwd, up, right), A the rest; cus: the device's compute units
hipError_t material_frame(const RenderArgs& R, const MaterialFrameArgs& A, const CollideWorld& Wd, uint32_t cus, hipStream_t stream);
#endif

}  // namespace vxrt
