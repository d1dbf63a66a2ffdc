// Host harness of the end-of-walk phase's continuation hook (vxrt_wave2.hpp: phase_end_deferred<STATS, HOOK>): ONE persistent
// tracer lane driven in the order of a round of k_render_persist2 -- tight-box phase, phase_end_deferred WITH a hook, the
// ray-finished phase, start_pending, probes.  The hook does what the render kernel's does: a first ray that has just ended on
// a voxel goes on, inside the phase, as a second ray from its hit point (+ a small step) along one FIXED direction, with that
// direction's per-ray invariants computed once and only for a start inside the coarse grid without a -0.0 component; every
// other first hit gets its second ray from begin_ray_deferred in the ray-finished phase.  Checked for every pair: the first
// ray's result as the hook reads it against the C oracle, and the second ray's result and probe counters against (a) a fresh
// tracer running begin_ray and the undeferred phases on that ray and (b) the C oracle.
// build: g++ -O1 -std=c++17 -ffp-contract=off -Itests/tools/hoststub -Ioracle tests/tools/host_end_hook_check.cpp oracle/vxo_*.c -lm -lpthread
// usage: host_end_hook_check world.bin n dx dy dz   (world.bin: int32 S, Sy, Sz, f, then the dense voxel words of the oracle)
#include "../voxelengine_amd/csrc/vxrt_wave2.hpp"
extern "C" {
#include "vxo.h"
}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace vxrt;

struct Ray { float o[3], d[3]; };

template <class TR>
static void trace_undeferred(TR& R, const WorldView& W, f3 o, f3 d, TraceResult& out)
{
    R.begin_ray(W, o, d, 2048);
    R.after_begin_ray(true);
    while (R.st != ST_DONE) {
        if (R.st == ST_BOX) R.template phase_box<true>(W);
        if (waits_for_end(R.st)) R.template phase_end<true>(W);
        R.template probe_pairs<1, true>(W);
    }
    R.result(W, out);
}

int main(int argc, char** argv)
{
    if (argc < 6) { printf("usage: host_end_hook_check world.bin n dx dy dz\n"); return 2; }
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[4];
    if (fread(hdr, 4, 4, fp) != 4) return 2;
    const int S = hdr[0], Sy = hdr[1], Sz = hdr[2], f = hdr[3];
    std::vector<uint32_t> dense((size_t)S * Sy * Sz / 32);
    if (fread(dense.data(), 4, dense.size(), fp) != dense.size()) return 2;
    fclose(fp);
    const int n = atoi(argv[2]);
    const f3 ldir = mk3((float)atof(argv[3]), (float)atof(argv[4]), (float)atof(argv[5]));
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
    W.c_wide = grid_is_wide(cx, cy, cz) ? 1 : 0;
    W.coarse_end = W.coarse_bits + coarse.size(); W.coarse_lo = coarse_pad.data(); W.coarse_hi = coarse_pad.data() + coarse_pad.size();
    W.pool_end = W.pool + pool.size(); W.pool_lo = pool_pad.data(); W.pool_hi = pool_pad.data() + pool_pad.size();
    if (W.c_wide) { printf("ordinary grids only\n"); return 2; }
    const float ext[3] = {(float)S, (float)Sy, (float)Sz};

    // first rays: from inside and around the grid, a share aimed at its centre so that rays from outside enter it
    srand(5);
    std::vector<Ray> rays(n);
    for (int i = 0; i < n; ++i) {
        Ray& r = rays[i];
        for (int a = 0; a < 3; ++a) {
            r.o[a] = (rand() / (float)RAND_MAX) * (i % 3 ? ext[a] : 3 * ext[a]) - (i % 3 ? 0 : ext[a]);
            r.d[a] = rand() / (float)RAND_MAX * 2 - 1;
        }
        if (i % 3 == 0 && i % 2 == 0) for (int a = 0; a < 3; ++a) r.d[a] = ext[a] * (0.25f + 0.5f * (rand() / (float)RAND_MAX)) - r.o[a];
        if (i % 7 == 0) r.d[i % 3] = 0;
        if (i % 11 == 0) { r.o[0] = floorf(r.o[0]); r.o[1] = floorf(r.o[1]); }
    }

    static uint32_t cold[CF_TRACER_FIELDS * 64], cold_ref[CF_TRACER_FIELDS * 64];
    // the fixed direction's per-ray invariants, by begin_ray_deferred itself (from a start inside the grid: no -0.0)
    WaveTracerT<false> Lt;
    Lt.init(W, cold_ref);
    Lt.begin_ray_deferred(W, mk3(0.5f * ext[0], 0.5f * ext[1], 0.5f * ext[2]), ldir, 2048);
    const bool dir_special = Lt.special;
    const f3 lstep = mk3(Lt.d.x * 0.01f, Lt.d.y * 0.01f, Lt.d.z * 0.01f);

    int bad = 0;
    unsigned long long first_hits = 0, from_hook = 0, from_next = 0, second_hits = 0, stray = 0;
    WaveTracerT<false> T;
    T.init(W, cold);
    int cur = -1, next = 0;
    bool second = false;     // the lane's ray is the second of its pair
    f3 o2 = mk3(0, 0, 0);    // ... which started here
    TraceResult first{};     // the first ray's result as the hook (or the ray-finished phase) read it
    auto check_first = [&](const TraceResult& t) {
        const Ray& r = rays[cur];
        int steps; float nn[3], pp[3] = {0, 0, 0}; int vox[3] = {0, 0, 0}; vxo_ray_stats st{};
        const int h = vxo_raytrace(w, 2048, r.o, r.d, &steps, nn, pp, vox, &st);
        bool ok = (t.hit == (h != 0)) && t.steps == steps;
        if (h) ok = ok && memcmp(&t.pos, pp, 12) == 0 && t.normal.x == nn[0] && t.normal.y == nn[1] && t.normal.z == nn[2] &&
                    t.vx == vox[0] && t.vy == vox[1] && t.vz == vox[2];
        if (!ok && bad++ < 5) printf("pair %d: first ray differs from the oracle (hit %d/%d steps %d/%d)\n", cur, (int)t.hit, h, t.steps, steps);
    };
    auto hook = [&](WaveTracerT<false>& Tr, const lanemask_t ended) -> lanemask_t {
        if (!lane_test(ended) || second || dir_special)
            return 0ull;
        if (Tr.st != ST_DONE) { printf("pair %d: a lane handed to the hook must be ST_DONE\n", cur); ++bad; }
        TraceResult r{};
        Tr.result(W, r);
        const f3 from = r.pos + lstep;
        const f3 s0 = mk3(from.x * W.inv_f, from.y * W.inv_f, from.z * W.inv_f);
        const uint32_t signs = __float_as_uint(s0.x) | __float_as_uint(s0.y) | __float_as_uint(s0.z);
        if (!((int32_t)signs >= 0 && s0.x < (float)W.cx && s0.y < (float)W.cy && s0.z < (float)W.cz))
            return 0ull;  // the ray-finished phase launches it
        first = r;
        check_first(r);
        first_hits += 1;
        from_hook += 1;
        second = true;
        o2 = from;
        Tr.cnt = RayCounters{0u, 0u, 0u};
        Tr.cold[CF_RAY_CODES * 64] = 2048u << 7;
        Tr.cold[CF_START_X * 64] = __float_as_uint(s0.x);
        Tr.cold[CF_START_Y * 64] = __float_as_uint(s0.y);
        Tr.cold[CF_START_Z * 64] = __float_as_uint(s0.z);
        Tr.cold[CF_LAST_CI * 64] = 0xFFFFFFFFu;
        Tr.cold[CF_TOTAL * 64] = 0u;
        Tr.d = Lt.d;
        Tr.ivx = Lt.ivx;
        Tr.ivy = Lt.ivy;
        Tr.ivz = Lt.ivz;
        Tr.dn = Lt.dn;
        Tr.special = false;
        Tr.st = ST_WALK;
        return 1ull;
    };
    for (;;) {
        if (T.st == ST_BOX) T.template phase_box<true>(W);
        if (waits_for_end(T.st)) {
            const bool was_second = second;
            T.template phase_end_deferred<true>(W, hook);
            if (second && !was_second && (T.st != ST_WALK || T.lane_fine() || !T.lane_pending())) {
                printf("pair %d: a lane the hook launched must be a pending coarse walker\n", cur);
                ++bad;
            }
        }
        if (T.st == ST_DONE) {
            bool launch_second = false;
            if (cur >= 0) {
                TraceResult t{};
                T.result(W, t);
                if (!second) {
                    check_first(t);
                    if (t.hit) {  // a first hit the hook left alone: its second ray by begin_ray_deferred
                        first_hits += 1;
                        from_next += 1;
                        first = t;
                        o2 = t.pos + lstep;
                        launch_second = true;
                    }
                } else {
                    // the second ray: a fresh tracer through begin_ray and the undeferred phases, and the oracle
                    WaveTracerT<false> R;
                    R.init(W, cold_ref);
                    TraceResult u{};
                    trace_undeferred(R, W, o2, ldir, u);
                    bool ok = t.hit == u.hit && t.steps == u.steps && T.cnt.coarse_probes == R.cnt.coarse_probes &&
                              T.cnt.brick_entries == R.cnt.brick_entries && T.cnt.fine_probes == R.cnt.fine_probes;
                    if (u.hit) ok = ok && memcmp(&t.pos, &u.pos, 12) == 0 && t.ncode == u.ncode && t.vx == u.vx && t.vy == u.vy && t.vz == u.vz;
                    const float oo[3] = {o2.x, o2.y, o2.z}, dd[3] = {ldir.x, ldir.y, ldir.z};
                    int steps; float nn[3], pp[3] = {0, 0, 0}; int vox[3] = {0, 0, 0}; vxo_ray_stats st{};
                    const int h = vxo_raytrace(w, 2048, oo, dd, &steps, nn, pp, vox, &st);
                    ok = ok && (t.hit == (h != 0)) && t.steps == steps && T.cnt.coarse_probes == st.coarse_probes &&
                         T.cnt.brick_entries == st.brick_entries && T.cnt.fine_probes == st.fine_probes && T.cnt.stray_loads == 0;
                    if (h) ok = ok && memcmp(&t.pos, pp, 12) == 0 && t.normal.x == nn[0] && t.normal.y == nn[1] && t.normal.z == nn[2] &&
                                t.vx == vox[0] && t.vy == vox[1] && t.vz == vox[2];
                    second_hits += t.hit ? 1 : 0;
                    stray += T.cnt.stray_loads;
                    if (!ok && bad++ < 5)
                        printf("pair %d: second ray from (%.9g,%.9g,%.9g): lane hit=%d steps=%d pos (%.9g,%.9g,%.9g) | begin_ray + phases hit=%d steps=%d "
                               "pos (%.9g,%.9g,%.9g) | oracle hit=%d steps=%d pos (%.9g,%.9g,%.9g)\n", cur, o2.x, o2.y, o2.z, (int)t.hit, t.steps,
                               t.pos.x, t.pos.y, t.pos.z, (int)u.hit, u.steps, u.pos.x, u.pos.y, u.pos.z, h, steps, pp[0], pp[1], pp[2]);
                    second = false;
                }
            }
            T.cnt = RayCounters{0u, 0u, 0u};
            if (launch_second) {
                second = true;
                T.begin_ray_deferred(W, o2, ldir, 2048);
            } else {
                if (next == n)
                    break;
                cur = next++;
                T.begin_ray_deferred(W, mk3(rays[cur].o[0], rays[cur].o[1], rays[cur].o[2]), mk3(rays[cur].d[0], rays[cur].d[1], rays[cur].d[2]), 2048);
            }
            T.after_begin_ray_deferred(true);
        }
        T.start_pending(W);
        T.template probe_pairs<3, true>(W);
    }
    if (host_unsuspected_exits() != 0) {
        printf("UNSUSPECTED EXITS: %llu\n", host_unsuspected_exits());
        bad += 1;
    }
    printf("mismatches %d of %d  (first hits %llu; second rays launched by the hook %llu, by the ray-finished phase %llu; second rays that hit %llu; "
           "direction special %d; loads outside the tables' slack %llu)\n", bad, n, first_hits, from_hook, from_next, second_hits, (int)dir_special, stray);
    return bad != 0;
}
