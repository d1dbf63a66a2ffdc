"""Shared scene/ray builders for the parity tests (seeded, small enough for the oracle to finish in seconds), the GPU test
helpers of the world queries (edits, reads, collision, islands, navigation) and the builder and runner of their host
harnesses (tests/tools/*_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAMERAS = {  # position as a fraction of the world size, euler angles
    "A": ((0.5, 0.9, 0.5), (-0.45, 0.7, 0.0)),
    "B": ((0.1, 1.2, 0.1), (-0.6, 3.9, 0.0)),      # outside the grid
    "C": ((0.5, 1.5, 0.5), (-1.5707, 0.0, 0.0)),   # top-down
    "D": ((0.02, 0.55, 0.5), (-0.05, 1.5707, 0.0)),  # grazing
}


def random_voxel_world(vxo, size=(64, 64, 64), factor=8, density=0.01, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.random(size) < density
    return vxo.World.from_voxels(v, factor)


def mixed_rays(dims, n, seed=0):
    """Origins inside / outside / on cell edges, directions random, axis-aligned and with zero components."""
    rng = np.random.default_rng(seed)
    X, Y, Z = dims
    o = np.empty((n, 3), np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 6
    o[:] = rng.random((n, 3)).astype(np.float32) * np.array([X, Y, Z], np.float32)          # inside
    o[k:2 * k] = (rng.random((k, 3)).astype(np.float32) * 3 - 1) * np.array([X, Y, Z], np.float32)  # in/outside
    o[2 * k:3 * k] = np.floor(o[2 * k:3 * k])                                                  # exact cell corners
    o[3 * k:4 * k, 0] = np.float32(X)                                                          # on the +x face
    d[3 * k:4 * k, 0] = -np.abs(d[3 * k:4 * k, 0])
    ax = rng.integers(0, 3, size=k)                                                            # axis-aligned
    d[4 * k:5 * k] = 0
    d[np.arange(4 * k, 5 * k), ax] = rng.choice([-1.0, 1.0], size=k).astype(np.float32)
    d[5 * k:6 * k, rng.integers(0, 3)] = 0                                                     # one zero component
    # aim a share of the outside rays at the grid so they enter it
    c = np.array([X, Y, Z], np.float32) / 2
    aim = slice(k, k + k // 2)
    d[aim] = (c + rng.normal(size=(k // 2, 3)).astype(np.float32) * c * 0.5) - o[aim]
    # adversarial families (every 13th/17th/... ray): tiny and denormal direction components, far-away origins
    # aimed at the grid, axis-aligned rays running exactly along cell boundaries
    idx = np.arange(n)
    m = idx % 13 == 0
    d[m, (idx[m] // 13) % 3] *= np.float32(1e-30)
    m = idx % 17 == 0
    d[m, (idx[m] // 17) % 3] = np.float32(1e-42)
    m = idx % 23 == 0
    o[m] = o[m] * np.float32(1000.0)
    d[m] = c - o[m]
    m = idx % 31 == 0                                 # exact x/y ties entering through a grid corner / far faces
    o[m, 0] = o[m, 1] = np.float32(X) * (1.5 + (idx[m] % 7)).astype(np.float32)
    d[m, 0] = d[m, 1] = -np.abs(d[m, 0]) - np.float32(0.1)
    m = idx % 37 == 0
    o[m, 1] = o[m, 2] = np.float32(-0.5 * Y)
    d[m, 1] = d[m, 2] = np.abs(d[m, 1]) + np.float32(0.1)
    m = idx % 29 == 0
    d[m] = 0
    d[m, 0] = np.where(idx[m] & 1, 1.0, -1.0).astype(np.float32)
    o[m, 1:] = np.floor(o[m, 1:])
    # a direction whose squared length underflows normalises to inf/NaN: not a ray (and float->int of NaN is
    # where host C and GPUs legitimately differ), so keep at least one ordinary component
    bad = (np.abs(d).max(axis=1) < 1e-10)
    d[bad] = (1, 0, 0)
    return o, d


def camera(name, dims, vxo_or_engine):
    (fx, fy, fz), euler = CAMERAS[name]
    pos = (fx * dims[0], fy * dims[1], fz * dims[2])
    f, u, r = vxo_or_engine.get_directions(euler) if hasattr(vxo_or_engine, "get_directions") \
        else vxo_or_engine.GetDirections(euler)
    return pos, f, u, r


def fibonacci_fan(n, origin):
    """n rays from one origin with Fibonacci-sphere directions: the 3-D analogue of the angular fan of the
    reference's 2-D tester (DDATestCpp/DDATestCpp.cpp:443-448, RAYS = 1000000 at :21).  Ray i points along
    (r cos(i*ga), 1 - (2i+1)/n, r sin(i*ga)), ga = the golden angle; evaluated in binary64, stored as binary32."""
    i = np.arange(n, dtype=np.float64)
    y = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - y * y)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), y, r * np.sin(phi)], 1).astype(np.float32)
    o = np.tile(np.asarray(origin, np.float32), (n, 1))
    return o, d


def float_bits(a):
    """binary32 array -> its bits as uint32, every NaN as the one canonical quiet NaN"""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


# ---- host harnesses of the world queries (tests/tools/*_check.cpp) -----------------------------------------------------
def build_harness(tmp_path_factory, name, *oracle_sources):
    """tests/tools/<name>.cpp compiled for the CPU through tests/tools/hoststub, with the oracle's brickmap builder and
    `oracle_sources` (file names under oracle/); returns the executable's path"""
    exe = str(tmp_path_factory.mktemp(name) / name)
    sources = ("vxo_trace.c", "vxo_world.c", "vxo_render.c") + oracle_sources
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "tools", "hoststub"),
                           "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(ROOT, "tests", "tools", name + ".cpp"),
                           "-x", "c", *[os.path.join(ROOT, "oracle", f) for f in sources], "-lm", "-lpthread", "-w"])
    return exe


def run_harness(exe, *args):
    """the harness run with `args`; asserts it passed ("ALL OK") and returns its stdout"""
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:]
    return out.stdout


def run_harness_files(exe, tmp_path, header, *arrays):
    """the harness run on in.bin (the int32 header, then the arrays' bytes); returns out.bin as bytes (uint8) and stdout"""
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.asarray(header, np.int32).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    stdout = run_harness(exe, inp, outp)
    return np.fromfile(outp, np.uint8), stdout


# ---- the GPU tests of the world queries ------------------------------------------------------------------------------
FRAME_W, FRAME_H = 64, 48
INV = float(np.float32(1.0) / np.sqrt(np.float32(3.0)))
BOX, SPHERE = 0, 1
FACADE_POSES = [((64.0, 230.0, 64.0), (-0.45, 0.7, 0.0)), ((70.5, 228.0, 66.0), (-0.5, 0.8, 0.0)),
                ((80.0, 220.25, 72.0), (-0.6, 1.0, 0.0))]


@pytest.fixture(scope="module")
def eng():
    import torch
    import voxelengine_amd as vx
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return vx, torch


def new_ctx(vx):
    c = vx.Context(0)
    c.SetEnvironment((INV, INV, INV), (2, 2, 2), (0.5, 0.5, 0.5))
    c.SetFOV(90.0)
    return c


def gen_dense(vxo, g, X, Y, Z):
    L = vxo.lib()
    p = L.vxo_gen_dense(g, X, Y, Z, 16)
    n = X * Y * Z // 32
    out = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), (n,)).copy()
    L.free(p)
    return out


def upload(ctx, w):
    ctx.upload_world(w.factor, w.cdims, w.coarse_bits, w.brick_slot, w.bounds, w.pool)


def assert_tables(ctx, w):
    """download_world against an oracle world, cell by cell: coarse bits, bounds, brick bits; slot numbers excluded"""
    d = ctx.download_world()
    assert tuple(d["cdims"]) == tuple(w.cdims) and d["factor"] == w.factor
    assert np.array_equal(d["coarse_bits"], w.coarse_bits)
    assert np.array_equal(d["bounds"].view(np.uint32), w.bounds.view(np.uint32))
    occ = w.brick_slot != 0xFFFFFFFF
    assert np.array_equal(d["brick_slot"] != 0xFFFFFFFF, occ)
    bw = w.factor ** 3 // 32
    got = d["pool"].reshape(-1, bw)[d["brick_slot"][occ]]
    want = w.pool.reshape(-1, bw)[w.brick_slot[occ]]
    assert np.array_equal(got, want)
    assert len(set(d["brick_slot"][occ].tolist())) == int(occ.sum())     # no slot shared by two cells
    return d


def render_frame(vx, ctx, torch, cam, dims, vxo, mode, variant=4):
    pos, f, u, r = camera(cam, dims, vxo)
    ctx.set_kernel_variant(variant)
    opts = vx.RenderOptions(shadow=True, bounce_samples=1, frame_number=3, mode=mode)
    if variant == 4:
        assert ctx.kernel_for_launch(FRAME_W, FRAME_H, opts) == 7
    fb = torch.zeros((FRAME_H, FRAME_W, 4), dtype=torch.uint8, device="cuda")
    ctx.RenderScreen(FRAME_W, FRAME_H, fb, pos, f, u, r, opts)
    ctx.set_kernel_variant(4)
    return fb.cpu().numpy()


def oracle_frame(vxo, w, cam, dims, mode):
    pos, f, u, r = camera(cam, dims, vxo)
    p = vxo.make_params(FRAME_W, FRAME_H, pos, f, u, r, frame_number=3, shadow=1, bounce_samples=1, mode=mode)
    return w.render(p, fb=np.zeros((FRAME_H, FRAME_W, 4), np.uint8), nthreads=16)["fb"]


def assert_frames(vx, ctx, torch, vxo, w, cams="ABCD", variants=(4, 1)):
    for cam in cams:
        for mode in (vx.MODE_SHADED, vx.MODE_DEBUG):
            want = oracle_frame(vxo, w, cam, w.dims, mode)
            for v in variants:
                assert np.array_equal(render_frame(vx, ctx, torch, cam, w.dims, vxo, mode, v), want), (cam, mode, v)


def assert_batch(ctx, w, n=3000, seed=0):
    o, d = mixed_rays(w.dims, n, seed)
    g = ctx.Raytrace(o, d)
    c = w.trace_batch(o, d, nthreads=16)
    assert np.array_equal(g["steps"], c["steps"]) and np.array_equal(g["voxel"], c["voxel"])
    assert np.array_equal(float_bits(g["hitPoint"]), float_bits(c["pos"]))
    assert np.array_equal(float_bits(g["normal"]), float_bits(c["normal"]))


def random_ops(rng, dims, n, rmax):
    ops = []
    for _ in range(n):
        if rng.random() < 0.5:
            lo = [int(rng.integers(-8, d + 8)) for d in dims]
            ops.append((BOX, int(rng.integers(0, 2)), lo, [l + int(rng.integers(-2, max(d // 3, 3))) for l, d in zip(lo, dims)]))
        else:
            c = [int(rng.integers(-10, d + 10)) for d in dims]
            ops.append((SPHERE, int(rng.integers(0, 2)), c, (int(rng.integers(0, rmax)), 0, 0)))
    return ops
