// Host harness of the deferred coarse starts of vxrt_wave2.hpp: ONE persistent tracer lane driven in the order of a round of
// k_render_persist2 / k_trace_batch_persist -- tight-box phase, phase_end_deferred, the ray-finished phase (result of the ray
// that ended, begin_ray_deferred + after_begin_ray_deferred for the next one), start_pending, probes -- against the C oracle.
// The lane lives across all rays, so whatever a ray or a deferred start leaves behind must not reach the next one.
// build: g++ -O1 -std=c++17 -ffp-contract=off -Itests/tools/hoststub -Ioracle tests/tools/host_defer_check.cpp oracle/vxo_*.c -lm -lpthread
#include "../voxelengine_amd/csrc/vxrt_wave2.hpp"
extern "C" {
#include "vxo.h"
}
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace vxrt;

struct Ray { float o[3], d[3]; };

// the adversarial ray families of host_wave_check.cpp: zero, tiny and denormal direction components, starts exactly on the far
// faces (edge rule), origins outside and far outside the grid, exact ties through corners, long and axis-parallel walks
static Ray make_ray(int i, const float ext[3], int Sy)
{
    Ray r;
    float* o = r.o;
    float* d = r.d;
    for (int a = 0; a < 3; ++a) { o[a] = (rand() / (float)RAND_MAX) * (i % 3 ? ext[a] : 3 * ext[a]) - (i % 3 ? 0 : ext[a]); d[a] = rand() / (float)RAND_MAX * 2 - 1; }
    if (i % 7 == 0) d[i % 3] = 0;
    if (i % 11 == 0) { o[0] = floorf(o[0]); o[1] = floorf(o[1]); }
    if (i % 13 == 0) d[(i / 13) % 3] *= 1e-30f;
    if (i % 17 == 0) d[(i / 17) % 3] = 1e-42f;
    if (i % 19 == 0) { o[(i / 19) % 3] = ext[(i / 19) % 3]; d[(i / 19) % 3] = -fabsf(d[(i / 19) % 3]) - 0.01f; }
    if (i % 23 == 0) { for (int a = 0; a < 3; ++a) { o[a] = o[a] * 1000.0f; d[a] = ext[a] * 0.5f - o[a]; } }
    if (i % 31 == 0) { o[0] = o[1] = Sy * (1.5f + (i % 7)); d[0] = d[1] = -fabsf(d[0]) - 0.1f; }
    if (i % 37 == 0) { o[1] = o[2] = -Sy * 0.5f; d[1] = d[2] = fabsf(d[1]) + 0.1f; }
    // long walks along whichever axes are more than 4 x the shortest, in turn (a grid long in x only: every such ray along x)
    int long_axes[3], n_long_axes = 0;
    for (int a = 0; a < 3; ++a) if (ext[a] > 4 * fminf(ext[0], fminf(ext[1], ext[2]))) long_axes[n_long_axes++] = a;
    if (i % 5 == 0 && n_long_axes) {
        const int a = long_axes[(i / 5) % n_long_axes];
        d[a] = (i & 8) ? 1.0f : -1.0f; d[(a + 1) % 3] *= 0.002f; d[(a + 2) % 3] *= 0.002f;
        if (i % 10 == 0) o[a] = d[a] > 0 ? -3.0f : ext[a] + 3.0f;
    }
    if (i % 29 == 0) { d[0] = (i & 1) ? 1.0f : -1.0f; d[1] = d[2] = 0; o[1] = floorf(o[1]); o[2] = floorf(o[2]); }
    if (i % 41 == 0) { int a = (i / 41) % 3; d[a] = (i & 2) ? 1.0f : -1.0f; d[(a + 1) % 3] *= 1e-4f; d[(a + 2) % 3] *= 1e-5f; o[a] = d[a] > 0 ? 0.0f : ext[a]; }
    // rays that miss the world altogether: the deferred start lands outside the grid and the lane meets the end-of-walk phase
    if (i % 43 == 0) { o[1] = -5.0f - (float)(i % 9); d[1] = -fabsf(d[1]) - 0.05f; }
    return r;
}

int main(int argc, char** argv)
{
    // usage: host_defer_check f S density n [Sy Sz [wide]]   (as host_wave_check)
    int f = argc > 1 ? atoi(argv[1]) : 8, S = argc > 2 ? atoi(argv[2]) : 64;
    double dens = argc > 3 ? atof(argv[3]) : 0.01;
    int n = argc > 4 ? atoi(argv[4]) : 30000;
    const int Sy = argc > 5 ? atoi(argv[5]) : S, Sz = argc > 6 ? atoi(argv[6]) : S;
    const int force_wide = argc > 7 ? atoi(argv[7]) : 0;
    std::vector<uint32_t> dense((size_t)S * Sy * Sz / 32, 0);
    srand(2);
    for (int z = 0; z < Sz; ++z) for (int y = 0; y < Sy; ++y) for (int x = 0; x < S; ++x)
        if (rand() / (double)RAND_MAX < dens) { uint64_t i = vxo_sample_index64(x, y, z, S, Sy); dense[i >> 5] |= 1u << (i & 31); }
    vxo_world* w = vxo_build_brickmap(dense.data(), S, Sy, Sz, f);
    // the oracle's tables in the order the tracer reads (linear x, z, y on both levels), with the addressable slack it needs
    const int cx = w->cdims[0], cy = w->cdims[1], cz = w->cdims[2];
    std::vector<uint2> meta(w->ncells);
    std::vector<uint32_t> coarse((w->ncells + 31) / 32, 0u);
    for (int z = 0; z < cz; ++z) for (int y = 0; y < cy; ++y) for (int x = 0; x < cx; ++x) {
        const uint64_t t = ref_tiled_index(x, y, z, cx / 8, cy / 8), i = hbm_index(x, y, z, cx, cz);
        uint32_t p = 0;
        if (w->brick_slot[t] != VXO_EMPTY_SLOT) for (int k = 0; k < 6; ++k) p |= (uint32_t)(int)w->bounds[t * 6 + k] << (5 * k);
        meta[i] = make_uint2(w->brick_slot[t], p);
        if ((w->coarse_bits[t >> 5] >> (t & 31)) & 1u) coarse[i >> 5] |= 1u << (i & 31);
    }
    const uint32_t bw = f * f * f / 32;
    std::vector<uint32_t> pool((size_t)w->nslots * bw, 0u);
    for (uint64_t s = 0; s < w->nslots; ++s)
        for (int z = 0; z < f; ++z) for (int y = 0; y < f; ++y) for (int x = 0; x < f; ++x) {
            const uint32_t t = ref_tiled_index(x, y, z, f / 8, f / 8), i = (uint32_t)hbm_index(x, y, z, f, f);
            if ((w->pool[s * bw + (t >> 5)] >> (t & 31)) & 1u) pool[s * bw + (i >> 5)] |= 1u << (i & 31);
        }
    const size_t cslack = (size_t)cx * cz / 32 + 1;
    std::vector<uint32_t> coarse_pad(coarse.size() + 2 * cslack, 0xA5A5A5A5u), pool_pad(pool.size() + 2 * (size_t)bw, 0x5A5A5A5Au);
    memcpy(coarse_pad.data() + cslack, coarse.data(), coarse.size() * 4);
    memcpy(pool_pad.data() + bw, pool.data(), pool.size() * 4);
    WorldView W{};
    W.coarse_bits = coarse_pad.data() + cslack; W.cell_meta = meta.data(); W.pool = pool_pad.data() + bw;
    W.cx = cx; W.cy = cy; W.cz = cz; W.c_row = cx; W.c_slice = cx * cz;
    W.f = f; W.f_row = f; W.f_slice = f * f; W.brick_words = bw; W.ff = (float)f; W.inv_f = 1.0f / f;
    W.wmax_x = (float)((double)W.cx - 1e-6); W.wmax_y = (float)((double)W.cy - 1e-6); W.wmax_z = (float)((double)W.cz - 1e-6);
    W.X = S; W.Y = Sy;
    W.c_wide = (force_wide || grid_is_wide(cx, cy, cz)) ? 1 : 0;
    W.coarse_end = W.coarse_bits + coarse.size(); W.coarse_lo = coarse_pad.data(); W.coarse_hi = coarse_pad.data() + coarse_pad.size();
    W.pool_end = W.pool + pool.size(); W.pool_lo = pool_pad.data(); W.pool_hi = pool_pad.data() + pool_pad.size();
    const float ext[3] = {(float)S, (float)Sy, (float)Sz};

    std::vector<Ray> rays(n);
    for (int i = 0; i < n; ++i) rays[i] = make_ray(i, ext, Sy);

    int bad = 0, n_hits = 0, n_long = 0, n_exhausted = 0;  // coverage: hits, walks beyond 1024 steps, rays that ran into MAX_STEPS
    unsigned long long stray = 0, slack = 0;
    // coverage: walks set up by start_pending for a new ray / for a restart after a brick miss, rounds in which it had nothing
    // to do, deferred starts that landed outside the grid
    unsigned long long starts_ray = 0, starts_restart = 0, idle_calls = 0, starts_outside = 0;
    static uint32_t cold[CF_TRACER_FIELDS * 64];
    auto run = [&](auto& T) {
        T.init(W, cold);  // st = ST_DONE: the lane starts by asking for a ray
        int cur = -1, next = 0;
        for (;;) {
            // ---- the cascade of a round: tight box, end of walk, ray finished
            if (T.st == ST_BOX) T.template phase_box<true>(W);
            bool restarted = false;
            if (waits_for_end(T.st)) {
                T.template phase_end_deferred<true>(W);
                restarted = T.pend_m != 0ull;
                if (restarted && (T.st != ST_WALK || T.lane_fine())) { printf("ray %d: a restarted lane must count as a coarse walker\n", cur); ++bad; }
            }
            if (T.st == ST_DONE) {
                if (cur >= 0) {
                    TraceResult t{};
                    T.result(W, t);
                    const Ray& r = rays[cur];
                    int steps; float nn[3], pp[3] = {0, 0, 0}; int vox[3] = {0, 0, 0}; vxo_ray_stats st{};
                    const int h = vxo_raytrace(w, 2048, r.o, r.d, &steps, nn, pp, vox, &st);
                    n_hits += h != 0; n_long += steps > 1024; n_exhausted += steps >= 2048 && !h;
                    bool ok = (t.hit == (h != 0)) && t.steps == steps && T.cnt.coarse_probes == st.coarse_probes &&
                              T.cnt.brick_entries == st.brick_entries && T.cnt.fine_probes == st.fine_probes && T.cnt.stray_loads == 0;
                    if (h) ok = ok && memcmp(&t.pos, pp, 12) == 0 && t.normal.x == nn[0] && t.normal.y == nn[1] && t.normal.z == nn[2] &&
                                t.vx == vox[0] && t.vy == vox[1] && t.vz == vox[2];
                    stray += T.cnt.stray_loads;
                    slack += T.cnt.slack_loads;
                    if (!ok && bad++ < 5)
                        printf("ray %d o=(%.9g,%.9g,%.9g) d=(%.9g,%.9g,%.9g) oracle hit=%d steps=%d probes=%llu/%llu/%llu pos (%.9g,%.9g,%.9g) vox (%d,%d,%d) | "
                               "lane hit=%d steps=%d probes=%u/%u/%u stray %u pos (%.9g,%.9g,%.9g) vox (%d,%d,%d)\n",
                               cur, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], h, steps, (unsigned long long)st.coarse_probes,
                               (unsigned long long)st.brick_entries, (unsigned long long)st.fine_probes, pp[0], pp[1], pp[2], vox[0], vox[1], vox[2],
                               (int)t.hit, t.steps, T.cnt.coarse_probes, T.cnt.brick_entries, T.cnt.fine_probes, T.cnt.stray_loads, t.pos.x, t.pos.y,
                               t.pos.z, t.vx, t.vy, t.vz);
                }
                if (next == n)
                    break;
                cur = next++;
                T.cnt = RayCounters{0u, 0u, 0u};
                T.begin_ray_deferred(W, mk3(rays[cur].o[0], rays[cur].o[1], rays[cur].o[2]), mk3(rays[cur].d[0], rays[cur].d[1], rays[cur].d[2]), 2048);
                T.after_begin_ray_deferred(true);
                starts_ray += 1;
            } else if (restarted) {
                starts_restart += 1;
            }
            // ---- the walks this round recorded, then the probes
            const bool pending = T.pend_m != 0ull;
            idle_calls += pending ? 0 : 1;
            T.start_pending(W);
            if (T.pend_m != 0ull || (pending && T.st != ST_WALK && T.st != ST_END)) { printf("ray %d: start_pending left the lane pending or in state %u\n", cur, T.st); ++bad; }
            starts_outside += (pending && T.st == ST_END) ? 1 : 0;
            T.template probe_pairs<3, true>(W);
        }
    };
    if (W.c_wide) { WaveTracerT<true> T; run(T); } else { WaveTracerT<false> T; run(T); }
    if (host_unsuspected_exits() != 0) {
        printf("UNSUSPECTED EXITS: %llu\n", host_unsuspected_exits());
        bad += 1;
    }
    printf("mismatches %d of %d  (hits %d, rays of more than 1024 steps %d, of 2048 or more without a hit %d; deferred starts: new rays %llu, restarts %llu, "
           "outside the grid %llu; rounds with nothing pending %llu; loads in the tables' slack %llu, outside it %llu)\n", bad, n, n_hits, n_long, n_exhausted, starts_ray, starts_restart, starts_outside, idle_calls, slack, stray);
    return bad != 0;
}
