"""Results recorded from the REFERENCE'S OWN CODE (tests/golden/ref_*.npz, generator: tests/golden/make_ref_golden.py).

The oracle (CPU) and the HIP path (GPU) must both reproduce them bit for bit.  Unlike tests/test_reference_pin.py these
need neither the reference's sources nor oracle/_ref: the inputs are rebuilt from seeds (tests/ref_pin_cases.py) and the
expected outputs are committed, so they run -- and never skip -- on every machine."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import helpers, ref_pin_cases as P

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(HERE, "golden", "make_ref_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

VARIANTS = ("checked_in", "shaded", "shaded_nocb", "shadow_s1", "shadow_s2", "shaded_s1", "shadow_s0", "ortho_shadow_s1")


def _load(name):
    return np.load(P.golden_path(name))


def _check_rays(g, ms, r, pos_key):
    assert np.array_equal(r["hit"], g["hit_%d" % ms]) and np.array_equal(r["steps"], g["steps_%d" % ms]), ms
    assert np.array_equal(helpers.float_bits(r["normal"]), helpers.float_bits(g["normal_%d" % ms].astype(np.float32))), ms
    assert np.array_equal(helpers.float_bits(r[pos_key]), g["pos_bits_%d" % ms]), ms


def _check_tables(g, name, factor, coarse_bits, brick_slot, bounds, pool):
    assert np.array_equal(coarse_bits, g[name + "_coarse_bits"])
    assert np.array_equal(helpers.float_bits(bounds.reshape(-1, 6)), helpers.float_bits(g[name + "_bounds"].astype(np.float32)))
    occ = brick_slot != 0xFFFFFFFF
    bricks = pool.reshape(-1, factor ** 3 // 32)[brick_slot[occ]]               # cell order; slot numbering excepted
    assert np.array_equal(G.brick_hashes(bricks), g[name + "_brick_sha256"])


def _frame_opts(sw):
    return dict(mode=sw.get("mode", 0), checkerboard=bool(sw.get("checkerboard", 0)), shadow=bool(sw.get("shadow", 0)),
                bounce_samples=sw.get("bounce_samples", 0), ortho=bool(sw.get("ortho", 0)))


def test_fixture_metadata():
    m = _load("ref_meta")
    man = json.loads(str(m["manifest"]))
    from oracle import ref_build
    assert man["sha256"] == ref_build.SHA256 and sorted(man["variants"]) == sorted(VARIANTS) == sorted(ref_build.VARIANTS)
    assert man["variants"] == json.loads(json.dumps(ref_build.manifest("x")["variants"]))     # the recorded edits are today's recipe
    assert "clean exit" in str(m["sanitizer"]) and str(m["sanitizer"]).count("no float cast out of range") >= 5 + len(VARIANTS)
    assert len(m["zero_x_seeds"]) == 193


@pytest.mark.parametrize("name", P.GOLDEN_RAY_WORLDS)
def test_oracle_reproduces_reference_rays(vxo, name):
    g = _load("ref_rays_" + name)
    o, d = P.golden_rays(name)
    assert str(g["inputs"]) == G.digest(o, d, P.dense(name)), "the seeded inputs changed"
    for ms in P.GOLDEN_MAX_STEPS:
        _check_rays(g, ms, P.oracle_world(name).trace_batch(o, d, max_steps=ms), "pos")
    assert 0 < int(g["hit_2048"].sum()) < len(o)                                 # hits and misses
    assert name == "dense8" or not np.array_equal(g["hit_2048"], g["hit_8"])     # (in the dense world 8 steps always suffice)


def test_oracle_reproduces_reference_builder(vxo):
    g = _load("ref_builder")
    for f, name in P.GOLDEN_BUILDER_WORLDS.items():
        assert str(g[name + "_inputs"]) == G.digest(P.dense(name)), "the seeded inputs changed"
        w = P.oracle_world(name)
        assert w.factor == f
        _check_tables(g, name, f, w.coarse_bits, w.brick_slot, w.bounds, w.pool)


@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_reproduces_reference_frames(vxo, variant):
    g = _load("ref_frames_" + variant)
    sw = json.loads(str(g["switches"]))
    w = P.oracle_world(G.GOLDEN_FRAME_WORLD)
    fbuf = np.full((P.FRAME_H, P.FRAME_W, 4), G.STALE, np.uint8)
    for n in P.FRAME_NUMBERS:
        w.render(G.frame_params(sw, n), fb=fbuf)
        assert np.array_equal(fbuf, g["fb_%d" % n]), n
    assert np.array_equal(g["fb_0"], g["fb_1"]) == (not sw.get("checkerboard"))   # only the checkerboard and the bounce seeds see the frame number
    assert sw.get("mode") or not (g["fb_1"] == G.STALE).all(axis=2)[1:].any()     # shaded: the pair leaves no row but row 0 unwritten


@pytest.fixture(scope="module")
def eng():
    import torch
    import voxelengine_amd as vx
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ctx = helpers.new_ctx(vx)
    yield vx, ctx, torch
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.GOLDEN_RAY_WORLDS)
def test_hip_reproduces_reference_rays(eng, vxo, name):
    vx, ctx, _ = eng
    g = _load("ref_rays_" + name)
    o, d = P.golden_rays(name)
    helpers.upload(ctx, P.oracle_world(name))
    try:
        for variant in (4, 1):
            ctx.set_kernel_variant(variant)
            for ms in P.GOLDEN_MAX_STEPS:
                ctx.set_batch_max_steps(ms)
                _check_rays(g, ms, ctx.Raytrace(o, d), "hitPoint")
    finally:
        ctx.set_batch_max_steps(2048)
        ctx.set_kernel_variant(4)


@pytest.mark.gpu
def test_hip_tables_reproduce_reference_builder(eng, vxo):
    """the reference builder's tables against the device's: made by the on-device builder for the terrain (the one golden
    world a generator makes); for the two random worlds, which no device generator makes, only the upload / download round
    trip of the oracle's tables is checked, not a builder"""
    vx, ctx, _ = eng
    g = _load("ref_builder")
    for f, name in P.GOLDEN_BUILDER_WORLDS.items():
        (X, Y, Z), _f = P.WORLDS[name]
        if name == "terrain32":
            ctx.build_world(vx.GEN_INT_TERRAIN, X, Y, Z, f)
        else:
            helpers.upload(ctx, P.oracle_world(name))
        d = ctx.download_world()
        _check_tables(g, name, f, d["coarse_bits"], d["brick_slot"], d["bounds"], d["pool"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_hip_reproduces_reference_frames(eng, vxo, variant):
    vx, ctx, torch = eng
    g = _load("ref_frames_" + variant)
    sw = json.loads(str(g["switches"]))
    helpers.upload(ctx, P.oracle_world(G.GOLDEN_FRAME_WORLD))
    try:
        for kv in (4, 1):
            ctx.set_kernel_variant(kv)
            fbuf = torch.full((P.FRAME_H, P.FRAME_W, 4), G.STALE, dtype=torch.uint8, device="cuda")
            for n in P.FRAME_NUMBERS:
                p = G.frame_params(sw, n)
                ctx.SetOrthoWindowSize(*p.ortho_size[:])
                ctx.RenderScreen(P.FRAME_W, P.FRAME_H, fbuf, p.origin[:], p.fwd[:], p.up[:], p.right[:],
                                 vx.RenderOptions(frame_number=n, **_frame_opts(sw)))
                assert np.array_equal(fbuf.cpu().numpy(), g["fb_%d" % n]), (kv, n)
    finally:
        ctx.set_kernel_variant(4)
