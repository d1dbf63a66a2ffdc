// Host harness of the probed coarse set-up of vxrt_wave2.hpp (start_pending_probed) and of the round order of
// k_render_persist2 built on it: ONE persistent tracer lane driven through end-of-walk phase (with a continuation hook, as
// host_end_hook_check.cpp) -> ray-finished phase (begin_ray_deferred) -> start_pending_probed -> tight-box phase -> probes.
// The set-up's probe parks a lane whose start cell is occupied before any burst has run, the tight-box phase takes it in
// the same round, and the burst that follows must find `fix` consumed for it while it still consumes the `fix` of a brick
// entry the tight-box phase has just made.  Checked for every ray, first rays and the second rays the hook or the
// ray-finished phase launch from their hits: hit, steps, position bits, normal code, voxel and the three probe counters
// against (a) a fresh tracer running begin_ray and the undeferred phases and (b) the C oracle.
// build: g++ -O1 -std=c++17 -ffp-contract=off -Itests/tools/hoststub -Ioracle tests/tools/host_start_probe_check.cpp oracle/vxo_*.c -lm -lpthread
// usage: host_start_probe_check world.bin n dx dy dz   (world.bin: int32 S, Sy, Sz, f, then the dense voxel words of the oracle)
#include "../voxelengine_amd/csrc/vxrt_wave2.hpp"
extern "C" {
#include "vxo.h"
}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace vxrt;

// faces: axes whose START component (coarse units) is put exactly on the grid's far face after the world entry -- begin_ray's
// entry test moves an origin on a far face of these small grids just inside (the world box ends 1e-6 before the face; from 64
// coarse cells on that rounds to the face itself and such starts do reach the set-up), so the harness writes CF_START_* itself,
// as a continuation hook may.  The oracle's Raytrace has no such entry: these rays are compared with the fresh tracer only.
struct Ray { float o[3], d[3]; int faces; };

// begin_ray_deferred, then the start's components of `faces` moved onto the far faces
template <class TR>
static void begin_on_faces(TR& R, const WorldView& W, f3 o, f3 d, int faces)
{
    R.begin_ray_deferred(W, o, d, 2048);
    if (faces & 1) R.cold[CF_START_X * 64] = __float_as_uint((float)W.cx);
    if (faces & 2) R.cold[CF_START_Y * 64] = __float_as_uint((float)W.cy);
    if (faces & 4) R.cold[CF_START_Z * 64] = __float_as_uint((float)W.cz);
}

template <class TR>
static void trace_undeferred(TR& R, const WorldView& W, f3 o, f3 d, int faces, TraceResult& out)
{
    if (faces) {
        begin_on_faces(R, W, o, d, faces);
        R.after_begin_ray_deferred(true);
        R.start_pending(W);
    } else {
        R.begin_ray(W, o, d, 2048);
        R.after_begin_ray(true);
    }
    while (R.st != ST_DONE) {
        if (R.st == ST_BOX) R.template phase_box<true>(W);
        if (waits_for_end(R.st)) R.template phase_end<true>(W);
        R.template probe_pairs<1, true>(W);
    }
    R.result(W, out);
}

static float frand() { return rand() / (float)RAND_MAX; }

int main(int argc, char** argv)
{
    if (argc < 6) { printf("usage: host_start_probe_check world.bin n dx dy dz\n"); return 2; }
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
    std::vector<int> occupied;  // the occupied coarse cells, x | y << 10 | z << 20
    for (int z = 0; z < cz; ++z) for (int y = 0; y < cy; ++y) for (int x = 0; x < cx; ++x) {
        const uint64_t t = ref_tiled_index(x, y, z, cx / 8, cy / 8), i = hbm_index(x, y, z, cx, cz);
        uint32_t p = 0;
        if (w->brick_slot[t] != VXO_EMPTY_SLOT) for (int k = 0; k < 6; ++k) p |= (uint32_t)(int)w->bounds[t * 6 + k] << (5 * k);
        meta[i] = make_uint2(w->brick_slot[t], p);
        if ((w->coarse_bits[t >> 5] >> (t & 31)) & 1u) {
            coarse[i >> 5] |= 1u << (i & 31);
            occupied.push_back(x | (y << 10) | (z << 20));
        }
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
    if (W.c_wide || occupied.empty()) { printf("ordinary grids with voxels only\n"); return 2; }
    const float ext[3] = {(float)S, (float)Sy, (float)Sz};

    // first rays, by family (i % 8)
    srand(7);
    std::vector<Ray> rays(n);
    for (int i = 0; i < n; ++i) {
        Ray& r = rays[i];
        r.faces = 0;
        for (int a = 0; a < 3; ++a) {
            r.o[a] = frand() * ext[a];
            r.d[a] = frand() * 2 - 1;
        }
        const int fam = i % 8, j = i / 8;
        if (fam == 0) {         // from around the grid, half of them aimed into it
            for (int a = 0; a < 3; ++a) r.o[a] = frand() * 3 * ext[a] - ext[a];
            if (j % 2 == 0) for (int a = 0; a < 3; ++a) r.d[a] = ext[a] * (0.25f + 0.5f * frand()) - r.o[a];
        } else if (fam == 1 || fam == 2) {  // inside an occupied coarse cell: the set-up's probe parks the lane for the tight box
            const int c = occupied[(size_t)rand() % occupied.size()];
            const int cc[3] = {c & 1023, (c >> 10) & 1023, c >> 20};
            for (int a = 0; a < 3; ++a) r.o[a] = ((float)cc[a] + frand()) * (float)f;
        } else if (fam == 3) {  // exactly on one, two or all three far faces, moving in (edge rule: fix, single-step mode)
            const int faces = 1 + j % 3;
            for (int k = 0; k < faces; ++k) {
                const int a = (j / 3 + k) % 3;
                r.o[a] = ext[a];
                r.d[a] = -fabsf(r.d[a]) - 0.01f;
                r.faces |= 1 << a;
            }
            if (j % 2) {        // ... on a cell boundary of another axis too, and with the face's axis the slowest
                const int a = (j / 3) % 3;
                r.o[(a + 1) % 3] = floorf(r.o[(a + 1) % 3]);
                if (j % 4 == 1) r.d[a] *= 0.05f;
            }
        } else if (fam == 4) {  // outside the grid and moving away: the deferred start lands outside, nothing is probed
            const int a = j % 3;
            r.o[a] = (j & 4) ? -5.0f - (float)(j % 9) : ext[a] + 3.0f + (float)(j % 9);
            r.d[a] = (j & 4) ? -fabsf(r.d[a]) - 0.05f : fabsf(r.d[a]) + 0.05f;
        } else if (fam == 5) {  // `special`: a zero component, a component below 2^-40, a -0.0 start component
            const int a = j % 3;
            if (j % 4 == 0) r.d[a] = 0.0f;
            else if (j % 4 == 1) r.d[a] = (j & 8) ? 1e-13f : -1e-13f;
            else if (j % 4 == 2) { r.o[a] = -0.0f; r.d[a] = fabsf(r.d[a]) + 0.01f; }
            else { r.d[a] = (j & 8) ? 1.0f : -1.0f; r.d[(a + 1) % 3] = r.d[(a + 2) % 3] = 0.0f; }
            if (j % 8 >= 4) {   // ... starting inside an occupied cell
                const int c = occupied[(size_t)rand() % occupied.size()];
                const int cc[3] = {c & 1023, (c >> 10) & 1023, c >> 20};
                for (int b = 0; b < 3; ++b) if (!(j % 4 == 2 && b == a)) r.o[b] = ((float)cc[b] + frand()) * (float)f;
            }
        } else if (fam == 6) {  // on integer voxel coordinates
            r.o[0] = floorf(r.o[0]);
            r.o[1] = floorf(r.o[1]);
        }                       // fam == 7: anywhere inside
    }

    static uint32_t cold[CF_TRACER_FIELDS * 64], cold_ref[CF_TRACER_FIELDS * 64];
    // the fixed direction's per-ray invariants, by begin_ray_deferred itself (from a start inside the grid: no -0.0)
    WaveTracerT<false> Lt;
    Lt.init(W, cold_ref);
    Lt.begin_ray_deferred(W, mk3(0.5f * ext[0], 0.5f * ext[1], 0.5f * ext[2]), ldir, 2048);
    const bool dir_special = Lt.special;
    const f3 lstep = mk3(Lt.d.x * 0.01f, Lt.d.y * 0.01f, Lt.d.z * 0.01f);

    int bad = 0;
    // coverage: walks the set-up served, of them: start cell occupied (parked by the set-up's probe), then the tight box hit /
    // missed in the same round; ended by the set-up's probe (suspected or left); started with fix != 0 / in single-step mode /
    // outside the grid; special rays; second rays by the hook / by the ray-finished phase; bursts that consumed a brick
    // entry's fix
    unsigned long long walks = 0, occ = 0, box_hit = 0, box_miss = 0, ended = 0, n_fix = 0, n_single = 0, n_outside = 0, n_special = 0,
                       from_hook = 0, from_next = 0, brick_fix = 0, hits = 0, stray = 0;
    WaveTracerT<false> T;
    T.init(W, cold);
    int cur = -1, next = 0;
    bool second = false;            // the lane's ray is the second of its pair
    f3 o1 = mk3(0, 0, 0), d1 = o1;  // the lane's ray
    int faces1 = 0;                 // ... and the far faces its start was put on
    // the ray the lane has just finished, as read by whoever reads it (the hook or the ray-finished phase), against both references
    auto check = [&](const TraceResult& t, const RayCounters& c) {
        WaveTracerT<false> R;
        R.init(W, cold_ref);
        TraceResult u{};
        trace_undeferred(R, W, o1, d1, faces1, u);
        bool ok = t.hit == u.hit && t.steps == u.steps && c.coarse_probes == R.cnt.coarse_probes && c.brick_entries == R.cnt.brick_entries &&
                  c.fine_probes == R.cnt.fine_probes;
        if (u.hit) ok = ok && memcmp(&t.pos, &u.pos, 12) == 0 && t.ncode == u.ncode && t.vx == u.vx && t.vy == u.vy && t.vz == u.vz;
        const float oo[3] = {o1.x, o1.y, o1.z}, dd[3] = {d1.x, d1.y, d1.z};
        int steps; float nn[3], pp[3] = {0, 0, 0}; int vox[3] = {0, 0, 0}; vxo_ray_stats st{};
        int h = vxo_raytrace(w, 2048, oo, dd, &steps, nn, pp, vox, &st);
        if (faces1) {  // (no oracle for a start written behind the world entry: the fresh tracer stands in)
            h = u.hit; steps = u.steps; st.coarse_probes = R.cnt.coarse_probes; st.brick_entries = R.cnt.brick_entries; st.fine_probes = R.cnt.fine_probes;
            memcpy(pp, &u.pos, 12); nn[0] = u.normal.x; nn[1] = u.normal.y; nn[2] = u.normal.z; vox[0] = u.vx; vox[1] = u.vy; vox[2] = u.vz;
        }
        ok = ok && (t.hit == (h != 0)) && t.steps == steps && c.coarse_probes == st.coarse_probes && c.brick_entries == st.brick_entries &&
             c.fine_probes == st.fine_probes && c.stray_loads == 0;
        if (h) ok = ok && memcmp(&t.pos, pp, 12) == 0 && t.normal.x == nn[0] && t.normal.y == nn[1] && t.normal.z == nn[2] &&
                    t.vx == vox[0] && t.vy == vox[1] && t.vz == vox[2];
        hits += t.hit ? 1 : 0;
        stray += c.stray_loads;
        if (!ok && bad++ < 5)
            printf("ray %d%s o=(%.9g,%.9g,%.9g) d=(%.9g,%.9g,%.9g): lane hit=%d steps=%d probes %u/%u/%u pos (%.9g,%.9g,%.9g) | begin_ray + phases "
                   "hit=%d steps=%d probes %u/%u/%u pos (%.9g,%.9g,%.9g) | oracle hit=%d steps=%d probes %llu/%llu/%llu pos (%.9g,%.9g,%.9g)\n",
                   cur, second ? " (second)" : "", o1.x, o1.y, o1.z, d1.x, d1.y, d1.z, (int)t.hit, t.steps, c.coarse_probes, c.brick_entries,
                   c.fine_probes, t.pos.x, t.pos.y, t.pos.z, (int)u.hit, u.steps, R.cnt.coarse_probes, R.cnt.brick_entries, R.cnt.fine_probes,
                   u.pos.x, u.pos.y, u.pos.z, h, steps, (unsigned long long)st.coarse_probes, (unsigned long long)st.brick_entries,
                   (unsigned long long)st.fine_probes, pp[0], pp[1], pp[2]);
    };
    auto hook = [&](WaveTracerT<false>& Tr, const lanemask_t ended_m) -> lanemask_t {
        if (!lane_test(ended_m) || second || dir_special)
            return 0ull;
        if (Tr.st != ST_DONE) { printf("ray %d: a lane handed to the hook must be ST_DONE\n", cur); ++bad; }
        TraceResult r{};
        Tr.result(W, r);
        const f3 from = r.pos + lstep;
        const f3 s0 = mk3(from.x * W.inv_f, from.y * W.inv_f, from.z * W.inv_f);
        const uint32_t signs = __float_as_uint(s0.x) | __float_as_uint(s0.y) | __float_as_uint(s0.z);
        if (!((int32_t)signs >= 0 && s0.x < (float)W.cx && s0.y < (float)W.cy && s0.z < (float)W.cz))
            return 0ull;  // the ray-finished phase launches it
        check(r, Tr.cnt);
        from_hook += 1;
        second = true;
        o1 = from;
        d1 = ldir;
        faces1 = 0;
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
        // ---- end of walk, ray finished
        if (waits_for_end(T.st))
            T.template phase_end_deferred<true>(W, hook);
        if (T.st == ST_DONE) {
            bool launch_second = false;
            if (cur >= 0) {
                TraceResult t{};
                T.result(W, t);
                check(t, T.cnt);
                if (!second && t.hit) {  // a first hit the hook left alone: its second ray by begin_ray_deferred
                    from_next += 1;
                    o1 = t.pos + lstep;
                    d1 = ldir;
                    faces1 = 0;
                    launch_second = true;
                }
                second = launch_second;
            }
            T.cnt = RayCounters{0u, 0u, 0u};
            if (!launch_second) {
                if (next == n)
                    break;
                cur = next++;
                o1 = mk3(rays[cur].o[0], rays[cur].o[1], rays[cur].o[2]);
                d1 = mk3(rays[cur].d[0], rays[cur].d[1], rays[cur].d[2]);
                faces1 = rays[cur].faces;
            }
            begin_on_faces(T, W, o1, d1, faces1);
            T.after_begin_ray_deferred(true);
        }
        // ---- the set-up with its probe
        const bool pending = T.pend_m != 0ull;
        bool parked = false;
        if (pending) {
            WaveTracerT<false> C = T;  // what the plain set-up makes of this start (ordinary grids: it writes no cold field)
            C.start_pending(W);
            walks += 1;
            n_fix += C.fix != 0u;
            n_single += C.st == ST_WALK && C.t_hi == -kInf;
            n_outside += C.st == ST_END;
            n_special += C.special;
            const bool walking = C.st == ST_WALK;
            T.template start_pending_probed<true>(W);
            // ... and the first probe of a burst behind it: the state start_pending_probed must leave, field by field
            C.template probe_one<true>(W, true);
            const bool same = T.st == C.st && T.idx == C.idx && T.rem == C.rem && T.rp == C.rp && T.rpp == C.rpp && T.fix == 0u &&
                              memcmp(&T.tn_x, &C.tn_x, 4) == 0 && memcmp(&T.tn_y, &C.tn_y, 4) == 0 && memcmp(&T.tn_z, &C.tn_z, 4) == 0 &&
                              memcmp(&T.tl, &C.tl, 4) == 0 && memcmp(&T.tp, &C.tp, 4) == 0 && memcmp(&T.t_hi, &C.t_hi, 4) == 0 &&
                              T.bits == C.bits && T.rem0 == C.rem0 && T.pend_m == 0ull;
            if (!same && bad++ < 5) printf("ray %d: start_pending_probed did not leave the state of start_pending + the first probe\n", cur);
            parked = T.st == ST_BOX;
            occ += parked;
            ended += walking && T.st == ST_END;
        } else {
            T.template start_pending_probed<true>(W);  // (nothing pending: must leave the lane alone)
        }
        // ---- tight box, in the same round for a lane the set-up's probe parked
        if (T.st == ST_BOX) {
            T.template phase_box<true>(W);
            if (parked) {
                box_hit += T.lane_fine();
                box_miss += !T.lane_fine() && T.st != ST_DONE;
            }
            brick_fix += T.lane_fine() && T.fix != 0u;
        }
        T.template probe_pairs<3, true>(W);
        if (T.fix != 0u) { printf("ray %d: fix left behind a burst\n", cur); ++bad; }
    }
    if (host_unsuspected_exits() != 0) {
        printf("UNSUSPECTED EXITS: %llu\n", host_unsuspected_exits());
        bad += 1;
    }
    printf("mismatches %d of %d  (hits %llu; walks set up %llu: start cell occupied %llu, tight box hit %llu, missed %llu; ended by the set-up's probe %llu; "
           "fix %llu, single-step %llu, outside the grid %llu, special %llu; second rays by the hook %llu, by the ray-finished phase %llu; "
           "brick entries with fix %llu; direction special %d; loads outside the tables' slack %llu)\n", bad, n, hits, walks, occ, box_hit, box_miss,
           ended, n_fix, n_single, n_outside, n_special, from_hook, from_next, brick_fix, (int)dir_special, stray);
    return bad != 0;
}
