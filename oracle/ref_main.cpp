/*
 * ref_main.cpp -- stand-alone runner of the reference driver (oracle/ref_driver.cpp) over a job file.
 *
 * oracle/ref_build.py links it with the reference objects compiled under -fsanitize=float-cast-overflow
 * -fno-sanitize-recover (oracle/_ref/vxref_check_<variant>, one per variant).  tests/golden/make_ref_golden.py writes the
 * inputs of the pin tests into job files and runs this program on them once: a clean exit shows that those inputs reach no
 * float -> integer cast whose value does not fit, i.e. none of the reference's undefined conversions (the ten that
 * oracle/ref_build.py routes through clamping conversions are no casts any more and are not seen).  It prints a count and
 * checks nothing else.
 *
 * Job file: records of int32 words (floats as their bits), each starting with a tag:
 *   1 X Y Z factor, then X*Y*Z/32 dense words            build this world (replaces the current one)
 *   2 n max_steps, then n*3 origins, n*3 directions      trace n rays through the current world
 *   3 W H frame_number, then 24 floats                   render a frame: fov, ortho size (2), camera (12), environment (9)
 *   4 n, then n*12 floats                                ray / box: start, direction, box min, box max per case
 *   5 n, then n seeds                                    hash and random float
 *   6 n, then n*3 floats                                 fBm at n points
 *   7 dx dy dz n max_steps has_region take_initial scale  single-level traversal of n rays over a grid of its own: then
 *       dx*dy*dz/32 words, 6 floats per cell if scale != 0, 6 region floats if has_region, n*3 starts, n*3 directions
 *   8 X Y Z                                              the world generator kernel over an X*Y*Z grid
 *   0                                                    end
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" {
void vxref_ray_aabb(size_t n, const float *start, const float *dir, const float *bmin, const float *bmax, uint8_t *hit, float *p,
                    float *nrm);
void *vxref_world_build(const uint32_t *dense_words, int X, int Y, int Z, int factor);
void vxref_world_free(void *h);
void vxref_trace(void *h, int max_steps, size_t n, const float *origins, const float *dirs, uint8_t *hit, int32_t *steps,
                 float *normal, float *pos);
void vxref_render(void *h, uint32_t W, uint32_t H, uint32_t frame_number, float fov, const float ortho_size[2], const float cam[12],
                  const float env[9], uint8_t *fb);
void vxref_hash(size_t n, const uint32_t *seeds, uint32_t *hashes, float *randoms);
void vxref_fbm(size_t n, const float *xyz, float *out);
void vxref_dda(const uint32_t *words, const int dims[3], size_t n, const float *start, const float *dir, const float *region,
               int max_steps, const float *cell_boxes, int cell_boxes_scale, int take_initial_step, uint8_t *hit, uint8_t *oob,
               int32_t *steps, float *hit_cell, float *point, float *next_cell, float *normal);
void vxref_populate(int X, int Y, int Z, uint32_t *words);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s job.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    auto words = [&](size_t n) {
        std::vector<int32_t> v(n);
        if (n && fread(v.data(), 4, n, f) != n) {
            fprintf(stderr, "short job file\n");
            exit(2);
        }
        return v;
    };
    void *world = nullptr;
    size_t rays = 0, frames = 0, small = 0;
    for (;;) {
        int tag = words(1)[0];
        if (tag == 0)
            break;
        if (tag == 1) {
            auto h = words(4);
            auto d = words((size_t)h[0] * h[1] * h[2] / 32);
            if (world)
                vxref_world_free(world);
            world = vxref_world_build((const uint32_t *)d.data(), h[0], h[1], h[2], h[3]);
        } else if (tag == 2 && world) {
            auto h = words(2);
            size_t n = h[0];
            auto o = words(3 * n), d = words(3 * n);
            std::vector<uint8_t> hit(n);
            std::vector<int32_t> steps(n);
            std::vector<float> nrm(3 * n), pos(3 * n);
            vxref_trace(world, h[1], n, (const float *)o.data(), (const float *)d.data(), hit.data(), steps.data(), nrm.data(), pos.data());
            rays += n;
        } else if (tag == 3 && world) {
            auto h = words(3);
            auto p = words(24);
            const float *q = (const float *)p.data();
            std::vector<uint8_t> fb((size_t)h[0] * h[1] * 4);
            vxref_render(world, h[0], h[1], h[2], q[0], q + 1, q + 3, q + 15, fb.data());
            frames++;
        } else if (tag == 4) {
            size_t n = words(1)[0];
            auto c = words(12 * n);
            std::vector<float> s(3 * n), d(3 * n), lo(3 * n), hi(3 * n), p(3 * n), nr(3 * n);
            std::vector<uint8_t> hit(n);
            const float *q = (const float *)c.data();
            for (size_t i = 0; i < n; i++)
                for (int a = 0; a < 3; a++)
                    s[3 * i + a] = q[12 * i + a], d[3 * i + a] = q[12 * i + 3 + a], lo[3 * i + a] = q[12 * i + 6 + a],
                              hi[3 * i + a] = q[12 * i + 9 + a];
            vxref_ray_aabb(n, s.data(), d.data(), lo.data(), hi.data(), hit.data(), p.data(), nr.data());
            small += n;
        } else if (tag == 5) {
            size_t n = words(1)[0];
            auto s = words(n);
            std::vector<uint32_t> h(n);
            std::vector<float> r(n);
            vxref_hash(n, (const uint32_t *)s.data(), h.data(), r.data());
            small += n;
        } else if (tag == 6) {
            size_t n = words(1)[0];
            auto p = words(3 * n);
            std::vector<float> out(n);
            vxref_fbm(n, (const float *)p.data(), out.data());
            small += n;
        } else if (tag == 7) {
            auto h = words(8);
            size_t cells = (size_t)h[0] * h[1] * h[2], n = h[3];
            auto g = words(cells / 32);
            auto boxes = words(h[7] ? cells * 6 : 0);
            auto region = words(h[5] ? 6 : 0);
            auto s = words(3 * n), d = words(3 * n);
            std::vector<uint8_t> hit(n), oob(n);
            std::vector<int32_t> steps(n);
            std::vector<float> a(3 * n), b(3 * n), c(3 * n), e(3 * n);
            vxref_dda((const uint32_t *)g.data(), h.data(), n, (const float *)s.data(), (const float *)d.data(),
                      h[5] ? (const float *)region.data() : nullptr, h[4], h[7] ? (const float *)boxes.data() : nullptr, h[7], h[6],
                      hit.data(), oob.data(), steps.data(), a.data(), b.data(), c.data(), e.data());
            rays += n;
        } else if (tag == 8) {
            auto h = words(3);
            std::vector<uint32_t> w((size_t)h[0] * h[1] * h[2] / 32);
            vxref_populate(h[0], h[1], h[2], w.data());
            small += (size_t)h[0] * h[1] * h[2];
        } else {
            fprintf(stderr, "bad record %d\n", tag);
            return 2;
        }
    }
    if (world)
        vxref_world_free(world);
    fclose(f);
    printf("vxref_check: %zu rays, %zu frames, %zu small cases, no float cast out of range\n", rays, frames, small);
    return 0;
}
