// Host harness of the frame denoiser (voxelengine_amd/csrc/vxrt_denoise.hpp: the limits and the workspace formula, the guide
// key, the record loads, the staging of a tile, the 25 taps of a pixel and the stores), compiled for the CPU through
// tests/tools/hoststub and run launch by launch, workgroup by workgroup and lane by lane, in either instantiation.  The
// harness restates what vxrt_denoise.hip adds around that code, which the GPU suite covers:
//   the launch sequence   iteration i reads buffer (i + 1) & 1 and writes buffer i & 1 of the workspace; the first reads the
//                         float3 input and the keys, the last writes the outputs; a single iteration whose output aliases its
//                         input is preceded by the pack into buffer 1;
//   the barrier           every lane of a workgroup stages before any lane of it filters;
//   the guide kernel      one lane per pixel, its ray handed in (the camera is the renderer's, covered on the GPU).
// Every index the code forms into an input, the workspace, an output or the LDS tile is checked against that array's size
// for that launch (an array the launch must not touch has size 0); the LDS tile is poisoned before every workgroup; the
// workspace and the outputs carry guards behind them.  Self-contained (no oracle code), so that a stand-alone sanitizer
// build is one compiler line.  Run by tests/test_denoise_host.py, which compares the outputs with tests/ref_denoise.py.
//
//   denoise_check in.bin out.bin
//   in:  i32 op, W, H, a, b, c, d, e
//   op 0 (filter): a = iterations, b = staged (1: STAGED wherever it exists), c = fb, d = alias (the output is the input
//        buffer), e = the bits of color_scale; then W * H * 3 f32 colours, W * H u32 keys
//        out: W * H * 3 f32, then (fb) W * H u32 BGRA8
//   op 1 (keys): a, b, c = X, Y, Z; then W * H i64 hit indices, W * H * 3 f32 origins, W * H * 3 f32 directions
//        out: W * H u32 keys
//   op 2 (limits; nothing is read beyond the header): out: u32 accepted, u32 0, u64 workspace bytes
//   stdout: indices checked, "ALL OK" or "FAILED"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
static uint64_t checked = 0;
static uint64_t g_size[16];
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            if (fails < 20)                                         \
                printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                \
        }                                                           \
    } while (0)
static bool check_index(int array, uint64_t index)
{
    ++checked;
    if (index < g_size[array])
        return true;
    if (fails < 20)
        printf("FAIL: index %llu of array %d (size %llu)\n", (unsigned long long)index, array, (unsigned long long)g_size[array]);
    ++fails;
    return false;
}
// an index outside its array ends the run before the access
#define VXRT_DN_CHECK(array, index)                   \
    do {                                              \
        if (!check_index(array, (uint64_t)(index))) { \
            printf("FAILED\n");                       \
            exit(1);                                  \
        }                                             \
    } while (0)

#include <cstdlib>

#include "../../voxelengine_amd/csrc/vxrt_denoise.hpp"
using namespace vxrt;

template <bool STAGED, bool FIRST>
static void launch(const DenoiseArgs& A)
{
    uint32_t gx, gy;
    dn_grid(A.W, A.H, STAGED, gx, gy);
    CHECK(gx >= 1u && gy >= 1u && gy <= 65535u);
    std::vector<DnRec> tile(kDnLdsRecords);
    g_size[kDnLds] = STAGED ? dn_tile_width(A.step) * dn_tile_height(A.step) : 0u;
    CHECK(g_size[kDnLds] <= kDnLdsRecords);
    for (uint32_t by = 0; by < gy; ++by)
        for (uint32_t bx = 0; bx < gx; ++bx) {
            const DnRec poison{-1.0f, -2.0f, -3.0f, 0xDEADBEEFu};  // a key no pixel has: bit 31 set, axis 7
            for (auto& r : tile)
                r = poison;
            if (STAGED)
                for (uint32_t tid = 0; tid < 256u; ++tid)
                    dn_stage<FIRST>(A, bx, by, tid, tile.data());
            for (uint32_t tid = 0; tid < 256u; ++tid)
                dn_compute<STAGED, FIRST>(A, bx, by, tid, tile.data());
        }
}

static int run_filter(const int32_t* hd, FILE* in, const char* out_path)
{
    const uint32_t W = (uint32_t)hd[1], H = (uint32_t)hd[2];
    const int32_t iterations = hd[3];
    const bool staged = hd[4] != 0, fb = hd[5] != 0, alias = hd[6] != 0;
    float k;
    memcpy(&k, &hd[7], 4);
    if (!denoise_frame_ok(W, H) || iterations < 1 || iterations > kDnMaxIterations || !(k >= 0.0f)) {
        printf("outside the contract\n");
        return 2;
    }
    const uint64_t n = (uint64_t)W * H;
    const uint32_t guard = 0x5A5A5A5Au;
    std::vector<float> cin(3u * n + 1u), cout_(3u * n + 1u);
    std::vector<uint32_t> keys(n + 1u), fbv(n + 1u, guard);
    if (fread(cin.data(), 4, 3u * n, in) != 3u * n || fread(keys.data(), 4, n, in) != n)
        return 2;
    memcpy(&cin[3u * n], &guard, 4);
    memcpy(&cout_[3u * n], &guard, 4);
    keys[n] = guard;
    CHECK(denoise_workspace_bytes(W, H) == 2u * n * 16u);
    std::vector<DnRec> work(2u * n + 1u, DnRec{0.0f, 0.0f, 0.0f, guard});
    DnRec* const buf[2] = {work.data(), work.data() + n};

    DenoiseArgs A{};
    A.color_in = cin.data();
    A.keys = keys.data();
    A.color_out = alias ? cin.data() : cout_.data();
    A.fb = fb ? fbv.data() : nullptr;
    A.W = W;
    A.H = H;
    A.k = k;
    bool packed = false;
    if (iterations == 1 && alias) {  // k_denoise_pack, restated
        for (uint64_t i = 0; i < n; ++i)
            buf[1][i] = DnRec{cin[3u * i], cin[3u * i + 1u], cin[3u * i + 2u], keys[i]};
        packed = true;
    }
    for (int32_t i = 0; i < iterations; ++i) {
        A.step = 1u << i;
        A.last = i == iterations - 1;
        A.src = buf[(i + 1) & 1];
        A.dst = buf[i & 1];
        const bool first = i == 0 && !packed, st = staged && A.step <= kDnMaxStagedStep;
        g_size[kDnColorIn] = first ? 3u * n : 0u;
        g_size[kDnKeys] = first ? n : 0u;
        g_size[kDnSrc] = first ? 0u : n;
        g_size[kDnDst] = A.last ? 0u : n;
        g_size[kDnColorOut] = A.last ? 3u * n : 0u;
        g_size[kDnFb] = A.last && fb ? n : 0u;
        if (st)
            first ? launch<true, true>(A) : launch<true, false>(A);
        else
            first ? launch<false, true>(A) : launch<false, false>(A);
    }
    uint32_t g[4];
    memcpy(&g[0], &cin[3u * n], 4);
    memcpy(&g[1], &cout_[3u * n], 4);
    g[2] = keys[n];
    g[3] = fbv[n];
    for (int i = 0; i < 4; ++i)
        CHECK(g[i] == guard);
    CHECK(work[2u * n].key == guard);
    if (!fb)
        for (uint64_t i = 0; i < n; ++i)
            CHECK(fbv[i] == guard);
    if (iterations == 1 && !alias)  // one fused launch touches no workspace
        for (uint64_t i = 0; i < 2u * n; ++i)
            CHECK(work[i].key == guard);

    FILE* out = fopen(out_path, "wb");
    if (!out)
        return 2;
    fwrite(alias ? cin.data() : cout_.data(), 4, 3u * n, out);
    if (fb)
        fwrite(fbv.data(), 4, n, out);
    fclose(out);
    return 0;
}

static int run_keys(const int32_t* hd, FILE* in, const char* out_path)
{
    const uint32_t W = (uint32_t)hd[1], H = (uint32_t)hd[2], X = (uint32_t)hd[3], Y = (uint32_t)hd[4], Z = (uint32_t)hd[5];
    const uint64_t n = (uint64_t)W * H;
    std::vector<long long> hit(n);
    std::vector<float> o(3u * n), d(3u * n);
    if (fread(hit.data(), 8, n, in) != n || fread(o.data(), 4, 3u * n, in) != 3u * n || fread(d.data(), 4, 3u * n, in) != 3u * n)
        return 2;
    CHECK(X <= kDnMaxAxis && Y <= kDnMaxAxis && Z <= kDnMaxAxis);
    std::vector<uint32_t> keys(n);
    for (uint64_t i = 0; i < n; ++i) {
        keys[i] = guide_key(hit[i], X, Y, Z, &o[3u * i], &d[3u * i]);
        CHECK(keys[i] == 0u || ((keys[i] >> 31) == 1u && ((keys[i] >> 26) & 31u) <= 2u));
    }
    FILE* out = fopen(out_path, "wb");
    if (!out)
        return 2;
    fwrite(keys.data(), 4, n, out);
    fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: denoise_check in.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    int32_t hd[8];
    if (!in || fread(hd, 4, 8, in) != 8)
        return 2;
    int rc = 0;
    if (hd[0] == 0) {
        rc = run_filter(hd, in, argv[2]);
    } else if (hd[0] == 1) {
        rc = run_keys(hd, in, argv[2]);
    } else {
        const uint32_t ok = denoise_frame_ok((uint32_t)hd[1], (uint32_t)hd[2]) ? 1u : 0u, zero = 0u;
        const uint64_t bytes = denoise_workspace_bytes((uint32_t)hd[1], (uint32_t)hd[2]);
        FILE* out = fopen(argv[2], "wb");
        if (!out)
            return 2;
        fwrite(&ok, 4, 1, out);
        fwrite(&zero, 4, 1, out);
        fwrite(&bytes, 8, 1, out);
        fclose(out);
    }
    fclose(in);
    if (rc)
        return rc;
    printf("%llu indices checked, failures %d\n%s\n", (unsigned long long)checked, fails, fails ? "FAILED" : "ALL OK");
    return fails ? 1 : 0;
}
