/*
 * ref_driver.cpp -- C API over the REFERENCE's own functions, compiled as host C++ (oracle/ref_build.py).
 *
 * TEST INFRASTRUCTURE.  oracle/ref_build.py appends `#include "ref_driver.cpp"` to its temporary copy of the reference's
 * renderer source, so this file is the tail of that translation unit: it sees the renderer's file-local frame record and
 * compile-time switches without restating them, and every function below runs the reference's code, not a restatement.
 * One shared library is built per variant of the reference's compile-time switches (libvxref_<variant>.so); the Python side
 * is oracle/vxref.py.
 *
 * SINGLE-THREADED BY CONSTRUCTION: threadIdx, blockIdx, blockDim and gridDim are process globals here (on a GPU they are
 * per-thread registers), and the frame record and the environment are globals of the reference.  Never call two
 * functions of one library at the same time.  (The reference's brickmap builder starts its own std::threads; those do not
 * read the launch coordinates.)
 *
 * Nothing here calls the reference's brick upload: it copies from freed memory for empty bricks.  The tracer and the
 * renderer get the host brick array the builder returned.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>

#ifndef VXREF_VARIANT
#define VXREF_VARIANT "unnamed"
#endif

/* ---- the launch coordinates (device_launch_parameters.h declares them extern "C" through ref_shim.h) */
extern "C" {
uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
int warpSize = 32;

/* ---- the CUDA runtime calls the reference names, on the host heap */
cudaError_t cudaMalloc(void **p, size_t n)
{
    *p = malloc(n ? n : 1);
    return cudaSuccess;
}
cudaError_t cudaFree(void *p)
{
    free(p);
    return cudaSuccess;
}
cudaError_t cudaMemcpy(void *dst, const void *src, size_t n, enum cudaMemcpyKind)
{
    memcpy(dst, src, n);
    return cudaSuccess;
}
cudaError_t cudaDeviceSynchronize(void) { return cudaSuccess; }
cudaError_t cudaGetLastError(void) { return cudaSuccess; }
const char *cudaGetErrorString(cudaError_t) { return "host build: no CUDA runtime"; }
}

/* defined in the reference's world-builder source (its header also holds a kernel launch, so it is not included) */
float PerlinNoise(float x, float y, float z);
void PopulateVoxels(GPUDDA::BitArray voxels, uint3 size);

namespace {
inline float3 f3(const float *p) { return make_float3(p[0], p[1], p[2]); }
inline void put3(float *p, const float3 &v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }

GPUDDA::BitArray bits_from_words(const uint32_t *words, size_t nbits)
{
    GPUDDA::BitArray b(nbits, false);
    memcpy(b.Raw(), words, b.ByteSize());
    return b;
}

struct World {
    GPUDDA::VoxelBuffer3D dense, coarse;
    GPUDDA::VoxelBuffer3D *bricks;
    GPUDDA::Bounds3Df *boxes;
    int factor;
    size_t ncells;
};

void launch_at(unsigned x, unsigned y, unsigned z, unsigned bx, unsigned by, unsigned bz)
{
    blockDim = dim3(bx, by, bz);
    blockIdx = make_uint3(x / bx, y / by, z / bz);
    threadIdx = make_uint3(x % bx, y % by, z % bz);
}
} // namespace

extern "C" {

const char *vxref_variant(void) { return VXREF_VARIANT; }
int vxref_checkerboard(void) { return ENABLE_CHECKERBOARD_RENDER ? 1 : 0; }

/* ---- layout */
uint32_t vxref_sample_index(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t h)
{
    return GPUDDA::GetSampleIndex(x, y, z, w, h);
}
void vxref_position_from_index(uint32_t i, uint32_t w, uint32_t h, uint32_t *x, uint32_t *y, uint32_t *z)
{
    GPUDDA::GetPositionFromSampleIndex(i, w, h, *x, *y, *z);
}
/* every index of a w*h*d grid: index -> position -> index; pos = n*3, back = n */
void vxref_sample_index_sweep(uint32_t w, uint32_t h, uint32_t d, uint32_t *pos, uint32_t *back)
{
    for (uint32_t i = 0; i < w * h * d; i++) {
        GPUDDA::GetPositionFromSampleIndex(i, w, h, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
        back[i] = GPUDDA::GetSampleIndex(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], w, h);
    }
}

/* ---- ray / box: n cases of {start, dir, bmin, bmax}; p and nrm are pre-filled by the caller and written only on a hit */
void vxref_ray_aabb(size_t n, const float *start, const float *dir, const float *bmin, const float *bmax, uint8_t *hit,
                    float *p, float *nrm)
{
    for (size_t i = 0; i < n; i++) {
        float3 op = f3(p + 3 * i), on = f3(nrm + 3 * i);
        hit[i] = GPUDDA::RayIntersectsAABB(f3(start + 3 * i), f3(dir + 3 * i), f3(bmin + 3 * i), f3(bmax + 3 * i), &op, &on);
        put3(p + 3 * i, op), put3(nrm + 3 * i, on);
    }
}

/* ---- single-level traversal over a dense grid: n rays.  region = {min xyz, max xyz} or NULL; cell_boxes = 6 floats
 * per cell or NULL.  Outputs per ray: hit, out_of_bounds, steps, and the four vectors of the result record. */
void vxref_dda(const uint32_t *words, const int dims[3], size_t n, const float *start, const float *dir, const float *region,
               int max_steps, const float *cell_boxes, int cell_boxes_scale, int take_initial_step, uint8_t *hit, uint8_t *oob,
               int32_t *steps, float *hit_cell, float *point, float *next_cell, float *normal)
{
    GPUDDA::VoxelBuffer3D buf;
    size_t nbits = (size_t)dims[0] * dims[1] * dims[2];
    buf.grid = bits_from_words(words, nbits);
    for (int a = 0; a < 3; a++)
        buf.dimensions[a] = (uint16_t)dims[a];
    GPUDDA::Bounds3Df reg{};
    if (region)
        reg.min = f3(region), reg.max = f3(region + 3);
    for (size_t i = 0; i < n; i++) {
        auto P = GPUDDA::DDARayParams<float3, 3>::Default(buf, f3(start + 3 * i), f3(dir + 3 * i));
        P.bounds = region ? &reg : nullptr;
        P.max_steps = max_steps;
        P.per_voxel_bounds = (GPUDDA::Bounds3Df *)cell_boxes;
        P.per_voxel_bounds_scale = cell_boxes_scale;
        P.takeInitialStep = take_initial_step != 0;
        GPUDDA::DDARayResults<float3> R;
        memset(&R, 0, sizeof(R));
        GPUDDA::DDARayTraversal(P, R);
        hit[i] = R.hit, oob[i] = R.isOutOfBounds, steps[i] = R.stepsTaken;
        put3(hit_cell + 3 * i, R.HitCell), put3(point + 3 * i, R.HitIntersectedPoint);
        put3(next_cell + 3 * i, R.NextCell), put3(normal + 3 * i, R.HitNormal);
    }
    delete[] buf.grid.Raw();
}

/* ---- the brickmap builder on a dense tiled-linear bit grid */
void *vxref_world_build(const uint32_t *dense_words, int X, int Y, int Z, int factor)
{
    World *w = new World();
    w->dense.grid = bits_from_words(dense_words, (size_t)X * Y * Z);
    w->dense.dimensions[0] = (uint16_t)X, w->dense.dimensions[1] = (uint16_t)Y, w->dense.dimensions[2] = (uint16_t)Z;
    auto t = GPUDDA::GenerateLowresVoxelBuffer(w->dense, factor);
    w->coarse = std::get<0>(t), w->bricks = std::get<1>(t), w->boxes = std::get<2>(t);
    w->factor = factor;
    w->ncells = (size_t)(X / factor) * (Y / factor) * (Z / factor);
    return w;
}
void vxref_world_free(void *h)
{
    World *w = (World *)h;
    for (size_t i = 0; i < w->ncells; i++)
        if (w->bricks[i].dimensions[0] != 0) /* an empty brick's bits were freed by the builder itself */
            delete[] w->bricks[i].grid.Raw();
    delete[] w->bricks;
    delete[] w->boxes;
    delete[] w->coarse.grid.Raw();
    delete[] w->dense.grid.Raw();
    delete w;
}
/* coarse = ncells/32 words; boxes = ncells*6 floats {min xyz, max xyz}; brick_dims = ncells*3; bricks = ncells * f^3/32
 * words, cell by cell in the coarse grid's own index order, zero for a brick without bits */
void vxref_world_tables(void *h, uint32_t *coarse, float *boxes, uint16_t *brick_dims, uint32_t *bricks)
{
    World *w = (World *)h;
    size_t bw = (size_t)w->factor * w->factor * w->factor / 32;
    memcpy(coarse, w->coarse.grid.Raw(), w->coarse.grid.ByteSize());
    for (size_t i = 0; i < w->ncells; i++) {
        put3(boxes + 6 * i, w->boxes[i].min), put3(boxes + 6 * i + 3, w->boxes[i].max);
        for (int a = 0; a < 3; a++)
            brick_dims[3 * i + a] = w->bricks[i].dimensions[a];
        if (w->bricks[i].dimensions[0] != 0)
            memcpy(bricks + bw * i, w->bricks[i].grid.Raw(), bw * sizeof(uint32_t));
        else
            memset(bricks + bw * i, 0, bw * sizeof(uint32_t));
    }
}

/* ---- the two-level tracer over n rays; pos is pre-filled by the caller and written only on a hit (the reference writes
 * it only then); normal and steps are always written */
void vxref_trace(void *h, int max_steps, size_t n, const float *origins, const float *dirs, uint8_t *hit, int32_t *steps,
                 float *normal, float *pos)
{
    World *w = (World *)h;
    for (size_t i = 0; i < n; i++) {
        int s = 0;
        float3 nr = make_float3(0, 0, 0), p = f3(pos + 3 * i);
        hit[i] = GPUDDA::Raytrace(max_steps, f3(origins + 3 * i), f3(dirs + 3 * i), w->coarse, w->bricks, w->boxes, w->factor, s, nr, p);
        steps[i] = s;
        put3(normal + 3 * i, nr), put3(pos + 3 * i, p);
    }
}

/* ---- one frame: the setters, the frame record as the reference's frame call fills it (frame_number is the value the
 * kernel sees), then the pixel kernel once per thread of the launch grid that call would use.  fb = W*H*4 bytes, kept
 * where the launch writes nothing.  cam = origin, fwd, up, right; env = light direction, light colour, ambient. */
void vxref_render(void *h, uint32_t W, uint32_t H, uint32_t frame_number, float fov, const float ortho_size[2], const float cam[12],
                  const float env[9], uint8_t *fb)
{
    World *w = (World *)h;
    Graphics::Environment e;
    e.LightDirection = f3(env), e.LightColor = f3(env + 3), e.AmbientColor = f3(env + 6);
    Graphics::SetEnvironment(e);
    Graphics::SetFOV(fov);
    Graphics::SetOrthoWindowSize(make_float2(ortho_size[0], ortho_size[1]));
    hFrameInfo.Resolution = make_uint2(W, H);
    hFrameInfo.FrameNumber = frame_number;
    cudaMemcpyToSymbol(dFrameInfo, &hFrameInfo, sizeof(hFrameInfo));
    uint32_t rows = ENABLE_CHECKERBOARD_RENDER ? H >> 1 : H;
    const unsigned bx = 32;
    gridDim = dim3((W + bx - 1) / bx, rows, 1);
    for (uint32_t y = 0; y < rows; y++)
        for (uint32_t x = 0; x < gridDim.x * bx; x++) {
            launch_at(x, y, 0, bx, 1, 1);
            screenDispatch(f3(cam), f3(cam + 3), f3(cam + 6), f3(cam + 9), fb, &w->coarse, w->bricks, w->boxes, w->factor);
        }
}

/* ---- small functions */
void vxref_get_directions(const float euler[3], float fwd[3], float up[3], float right[3])
{
    float3 f, u, r;
    Graphics::GetDirections(f3(euler), &f, &u, &r);
    put3(fwd, f), put3(up, u), put3(right, r);
}
void vxref_hash(size_t n, const uint32_t *seeds, uint32_t *hashes, float *randoms)
{
    for (size_t i = 0; i < n; i++) {
        hashes[i] = cudaNoise::hash(seeds[i]);
        randoms[i] = cudaNoise::randomFloat(seeds[i]);
    }
}
void vxref_fbm(size_t n, const float *xyz, float *out)
{
    for (size_t i = 0; i < n; i++)
        out[i] = PerlinNoise(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}
/* the world generator kernel once per voxel of an X*Y*Z grid (its launch uses 8^3 blocks); words = X*Y*Z/32 */
void vxref_populate(int X, int Y, int Z, uint32_t *words)
{
    GPUDDA::BitArray b((size_t)X * Y * Z, false);
    memset(b.Raw(), 0, b.ByteSize());
    gridDim = dim3((X + 7) / 8, (Y + 7) / 8, (Z + 7) / 8);
    for (int z = 0; z < Z; z++)
        for (int y = 0; y < Y; y++)
            for (int x = 0; x < X; x++) {
                launch_at(x, y, z, 8, 8, 8);
                PopulateVoxels(b, make_uint3(X, Y, Z));
            }
    memcpy(words, b.Raw(), b.ByteSize());
    delete[] b.Raw();
}

} /* extern "C" */
