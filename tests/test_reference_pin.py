"""The oracle pinned to the REFERENCE'S OWN CODE, bit for bit, one unit at a time.

oracle/ref_build.py compiles the reference's sources as host C++ (oracle/_ref/libvxref_<variant>.so; loader oracle/vxref.py),
so "the source evaluated with IEEE binary32 semantics" -- the oracle's own definition -- is something that runs.  Every
test below feeds the same inputs to a reference function and to the oracle function that restates it and compares every
output of every ray, case or pixel; nothing is excluded by looking at a result.  The inputs hold no invalid ray (the rule
of include/vxrt.h), which the tests assert rather than filter; that they reach none of the reference's undefined
float -> int conversions is shown once by tests/golden/make_ref_golden.py (the driver under
-fsanitize=float-cast-overflow) and recorded in tests/golden/ref_meta.npz.

Where the reference's sources are on the machine but oracle/_ref is not, the tests fail and say how to build it; they skip
only where both are absent.  DESIGN.md section 2 lists what this pin does not cover.
"""
import ctypes as C

import numpy as np
import pytest

from tests import helpers, ref_pin_cases as P, render_edge_cases as rec

fb = helpers.float_bits


@pytest.fixture(scope="module")
def vxref():
    from oracle import vxref as m
    if not m.available():
        if m.reference_present():
            pytest.fail("oracle/_ref is missing or older than the recipe (oracle/ref_build.py, ref_shim.h, ref_driver.cpp) although the reference's sources are here: run `__graft_entry__.build()`")
        pytest.skip("neither the reference's sources nor an oracle/_ref built from this recipe are on this machine")
    return m


def _same(ref, got, keys, what):
    for k in keys:
        a, b = ref[k], got[k]
        if a.dtype.kind == "f":
            a, b = fb(a), fb(b)
        bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differs from the reference at %d of %d, first %s: reference %s, oracle %s" % (
            what, k, bad.size, len(a), bad[:5], ref[k][bad[:3]], got[k][bad[:3]])


# ---- sample index
@pytest.mark.parametrize("dims", [(8, 8, 8), (16, 8, 24), (24, 16, 8), (64, 8, 8)])
def test_sample_index_and_inverse(vxo, vxref, dims):
    w, h, d = dims
    pos, back = vxref.sample_index_sweep(w, h, d)
    n = w * h * d
    assert np.array_equal(back, np.arange(n, dtype=np.uint32))            # the reference's pair is a bijection here
    assert len({tuple(p) for p in pos}) == n and (pos < np.array(dims, np.uint32)).all()
    L = vxo.lib()
    for i in range(n):
        x, y, z = (int(c) for c in pos[i])
        assert vxo.position_from_index(i, w, h) == (x, y, z)
        assert L.vxo_sample_index(x, y, z, w, h) == i == vxref.sample_index(x, y, z, w, h)


# ---- ray / box
def _oracle_aabb(vxo, s, d, lo, hi):
    n = len(s)
    out = dict(hit=np.zeros(n, np.uint8), pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32))
    L, f32p = vxo.lib(), C.POINTER(C.c_float)
    ptr = [a.ctypes.data_as(f32p) for a in (s, d, lo, hi, out["pos"], out["normal"])]
    step = 3 * 4
    addr = [C.cast(p, C.c_void_p).value for p in ptr]
    for i in range(n):
        out["hit"][i] = L.vxo_ray_aabb(*[C.cast(a + i * step, f32p) for a in addr])
    return out


def test_ray_aabb(vxo, vxref):
    cases = [np.ascontiguousarray(np.concatenate([a, b])) for a, b in zip(P.aabb_cases(), P.quirk_aabb_cases())]
    s, d, lo, hi = cases
    assert len(s) >= 100000 and np.isfinite(s).all() and np.isfinite(d).all()
    ref = vxref.ray_aabb(s, d, lo, hi)
    got = _oracle_aabb(vxo, s, d, lo, hi)
    assert 0.2 < ref["hit"].mean() < 0.8
    _same(ref, got, ("hit", "pos", "normal"), "ray/box")


# ---- single-level traversal and the two-level tracer
def _trace_inputs(dims):
    o = np.concatenate([P.adversarial_rays(dims)[0], P.mixed_rays(dims)[0]])
    d = np.concatenate([P.adversarial_rays(dims)[1], P.mixed_rays(dims)[1]])
    assert rec._valid(o, d).all()                                          # asserted, not filtered
    return o, d


@pytest.mark.parametrize("name", sorted(P.WORLDS))
def test_raytrace(vxo, vxref, name):
    w, r = P.oracle_world(name), P.reference_world(name, vxref.DEFAULT)
    o, d = _trace_inputs(w.dims)
    assert len(o) == 103000
    for ms in P.MAX_STEPS:
        ref = r.trace(o, d, ms)
        got = w.trace_batch(o, d, max_steps=ms)
        if ms == 2048 and name != "dense8":
            assert 0 < int(ref["hit"].sum()) < len(o)
        _same(ref, got, ("hit", "steps", "normal", "pos"), "Raytrace %s maxSteps %d" % (name, ms))


def test_raytrace_quirk_cases(vxo, vxref):
    for name, (v, f, o, d, _) in P.quirk_inputs().items():
        assert rec._valid(o, d).all()
        w, r = vxo.World.from_voxels(v, f), vxref.World.from_voxels(v, f)
        for ms in P.MAX_STEPS:
            ref, got = r.trace(o, d, ms), w.trace_batch(o, d, max_steps=ms)
            _same(ref, got, ("hit", "steps", "normal", "pos"), "Raytrace %s maxSteps %d" % (name, ms))


def _oracle_dda(vxo, words, dims, s, d, *, region=None, max_steps=2048, cell_boxes=None, scale=0, take_initial_step=False):
    """oracle.vxo's vxo_dda over n rays (vxo_dda_batch), in the shape of vxref.dda"""
    s, d = np.ascontiguousarray(s, np.float32), np.ascontiguousarray(d, np.float32)
    n = len(s)
    out = dict(hit=np.zeros(n, np.uint8), out_of_bounds=np.zeros(n, np.uint8), steps=np.zeros(n, np.int32),
               hit_cell=np.zeros((n, 3), np.float32), point=np.zeros((n, 3), np.float32), next_cell=np.zeros((n, 3), np.float32),
               normal=np.zeros((n, 3), np.float32))
    words = np.ascontiguousarray(words, np.uint32)
    Pm = vxo.DDAParams()
    Pm.bits = words.ctypes.data_as(C.POINTER(C.c_uint32))
    Pm.nbits = dims[0] * dims[1] * dims[2]
    Pm.dims = (C.c_int * 3)(*dims)
    Pm.max_steps = max_steps
    Pm.take_initial_step = int(take_initial_step)
    if region is not None:
        Pm.has_bounds = 1
        Pm.bounds_min, Pm.bounds_max = (C.c_float * 3)(*region[:3]), (C.c_float * 3)(*region[3:])
    if cell_boxes is not None:
        cb = np.ascontiguousarray(cell_boxes, np.float32)
        Pm.cell_bounds, Pm.cell_bounds_scale = cb.ctypes.data_as(C.POINTER(C.c_float)), scale
    vxo.lib().vxo_dda_batch(C.byref(Pm), n, s.ctypes.data, d.ctypes.data, *[out[k].ctypes.data for k in DDA_KEYS])
    return out


DDA_KEYS = ("hit", "out_of_bounds", "steps", "hit_cell", "point", "next_cell", "normal")


def _dda_both(vxo, vxref, what, words, dims, s, d, **kw):
    ref = vxref.dda(words, dims, s, d, region=kw.get("region"), max_steps=kw.get("max_steps", 2048), cell_boxes=kw.get("cell_boxes"),
                    cell_boxes_scale=kw.get("scale", 0), take_initial_step=kw.get("take_initial_step", False))
    _same(ref, _oracle_dda(vxo, words, dims, s, d, **kw), DDA_KEYS, "DDA %s %s" % (what, {k: v for k, v in kw.items() if k != "cell_boxes"}))
    return ref


@pytest.mark.parametrize("name", sorted(P.WORLDS))
def test_dda_single_level(vxo, vxref, name):
    """DDARayTraversal alone on the inputs of test_raytrace (the 3000 adversarial rays and the 100k mixed rays, every step
    budget, all four worlds), in the two ways Raytrace uses it -- the coarse grid with the builder's per-cell boxes (rays
    in coarse-cell units) and a dense grid (rays in voxel units; here the whole world as one grid) -- and, on the
    adversarial rays, with the region check and with takeInitialStep, which Raytrace never sets.  Every field of the
    result record is compared; those the reference leaves unwritten start at zero on both sides."""
    (X, Y, Z), f = P.WORLDS[name]
    w = P.oracle_world(name)
    o, d = _trace_inputs((X, Y, Z))
    oc = np.ascontiguousarray(o / np.float32(f))
    for ms in P.MAX_STEPS:
        ref = _dda_both(vxo, vxref, name + " dense", P.dense(name), (X, Y, Z), o, d, max_steps=ms)
        refc = _dda_both(vxo, vxref, name + " coarse", w.coarse_bits, w.cdims, oc, d, max_steps=ms, cell_boxes=w.bounds, scale=f)
        if ms == 2048:
            assert ref["hit"].any() and not ref["hit"].all() and refc["hit"].any() and not refc["hit"].all()
    oa, da = P.adversarial_rays((X, Y, Z))
    region = P.dda_region((X, Y, Z))
    for ms in P.MAX_STEPS:
        for reg in (None, region):
            for tis in (False, True):
                if reg is not None or tis:
                    r = _dda_both(vxo, vxref, name + " dense", P.dense(name), (X, Y, Z), oa, da, max_steps=ms, region=reg, take_initial_step=tis)
                    assert reg is None or ms < 100 or r["out_of_bounds"].any()


def test_dda_quirk_cases(vxo, vxref):
    """every quirk case's ray through the single-level traversal of its own world: the coarse grid with boxes and the dense grid"""
    for name, (v, f, o, d, _) in P.quirk_inputs().items():
        w = vxo.World.from_voxels(v, f)
        o1, d1 = o.reshape(1, 3), d.reshape(1, 3)
        for ms in P.MAX_STEPS:
            _dda_both(vxo, vxref, name + " dense", vxo.dense_from_voxels(v), v.shape, o1, d1, max_steps=ms)
            _dda_both(vxo, vxref, name + " coarse", w.coarse_bits, w.cdims, o1 / np.float32(f), d1, max_steps=ms, cell_boxes=w.bounds, scale=f)
            _dda_both(vxo, vxref, name + " brick region", vxo.dense_from_voxels(v), v.shape, o1, d1, max_steps=ms,
                      region=(0.0, 0.0, 0.0, float(v.shape[0] - f), float(v.shape[1]), float(v.shape[2])))


# ---- builder
@pytest.mark.parametrize("name", sorted(P.builder_worlds()) + ["terrain32", "random16", "dense8"])
def test_builder(vxo, vxref, name):
    if name in P.WORLDS:
        (X, Y, Z), f = P.WORLDS[name]
        dense = P.dense(name)
    else:
        v, f = P.builder_worlds()[name]
        (X, Y, Z), dense = v.shape, vxo.dense_from_voxels(v)
    w = vxo.World.from_dense(dense, X, Y, Z, f)
    t = vxref.World(dense, X, Y, Z, f).tables()
    assert np.array_equal(t["coarse_bits"], w.coarse_bits)
    assert np.array_equal(fb(t["bounds"]), fb(w.bounds))
    occ = w.brick_slot != vxo.EMPTY_SLOT
    # a brick holds bits exactly where its coarse bit is set; the reference marks a brick without bits by dimensions 0
    cb = (w.coarse_bits[np.arange(w.ncells) // 32] >> (np.arange(w.ncells) % 32).astype(np.uint32)) & 1
    assert np.array_equal(occ, cb.astype(bool)) and np.array_equal(t["brick_dims"][:, 0] != 0, occ)
    assert (t["brick_dims"][occ] == f).all() and (t["brick_dims"][~occ] == 0).all()
    empty = np.array([0, 0, 0, -1, -1, -1], np.float32)
    assert (t["bounds"][~occ] == empty).all()
    bw = f ** 3 // 32
    assert np.array_equal(t["bricks"][occ], w.pool.reshape(-1, bw)[w.brick_slot[occ]])       # slot numbering excepted
    if name.startswith("empty"):
        assert not occ.any()
    if name.startswith("full"):
        assert occ.all() and (t["bricks"] == 0xFFFFFFFF).all()


# ---- small functions
def test_get_directions(vxo, vxref):
    hp = float(np.float32(np.pi / 2))
    eulers = [e for _, e in helpers.CAMERAS.values()] + [(0.0, 0.0, 0.0), (0.0, hp, 0.0), (0.0, -hp, 0.0), (hp, 0.0, 0.0),
                                                        (-hp, 0.0, 0.0), (hp, hp, 0.0), (-hp, -hp, 0.0)]
    for e in eulers:
        for a, b in zip(vxref.get_directions(e), vxo.get_directions(e)):
            assert np.array_equal(fb(a), fb(b)), e


def test_hash_and_random_float(vxo, vxref):
    """2^24 seeds in a stride across all 2^32, the ends of the range, and the 193 seeds whose random float makes a bounce
    direction's x component exactly 0 (tests/render_edge_cases.py; recorded by tests/golden/make_ref_golden.py, which finds
    them by running the reference's function over all 2^32 seeds)"""
    zero_x = np.load(P.golden_path("ref_meta"))["zero_x_seeds"]
    assert zero_x.dtype == np.uint32 and len(zero_x) == 193 and len(set(zero_x.tolist())) == 193
    seeds = np.concatenate([P.hash_seeds(), zero_x])
    h, r = vxref.hash_and_random(seeds)
    gh, gr = np.zeros(len(seeds), np.uint32), np.zeros(len(seeds), np.float32)
    vxo.lib().vxo_hash_batch(len(seeds), seeds.ctypes.data, gh.ctypes.data, gr.ctypes.data)
    assert np.array_equal(h, gh) and np.array_equal(fb(r), fb(gr))
    assert (r[-193:] * np.float32(2) - np.float32(1) == 0).all()
    assert vxo.hash32(int(seeds[5])) == int(h[5]) and vxo.random_float(int(seeds[5])) == float(r[5])     # the scalar entries


def test_fbm_perlin(vxo, vxref):
    p = P.fbm_points()
    assert len(p) == 100000
    ref = vxref.fbm(p)
    L = vxo.lib()
    got = np.fromiter((L.vxo_fbm_perlin(float(x), float(y), float(z)) for x, y, z in p), np.float32, count=len(p))
    assert np.array_equal(fb(ref), fb(got)) and np.isfinite(ref).all() and ref.std() > 0


def test_populate_voxels(vxo, vxref):
    ref = vxref.populate(64, 64, 64)
    got = helpers.gen_dense(vxo, vxo.GEN_PERLIN_REF, 64, 64, 64)
    assert np.array_equal(ref, got) and 0 < int(np.unpackbits(ref.view(np.uint8)).sum()) < 64 ** 3


# ---- frames
def _frame_pair(vxref, variant, world_name, camera, W, H, frames, **kw):
    """(reference frames, oracle frames): the variant's bytes after each frame number in sequence on one buffer"""
    sw = vxref.switches(variant)
    r, w = P.reference_world(world_name, variant), P.oracle_world(world_name)
    fr, fo = np.full((H, W, 4), 77, np.uint8), np.full((H, W, 4), 77, np.uint8)
    out = []
    for n in frames:
        p = P.make_params(W, H, camera, sw, n, **kw)
        env = dict(light_dir=p.env.light_dir[:], light_color=p.env.light_color[:], ambient=p.env.ambient[:])
        r.render(W, H, n, p.origin[:], p.fwd[:], p.up[:], p.right[:], fb=fr, fov=p.fov_deg, ortho_size=p.ortho_size[:], **env)
        w.render(p, fb=fo)
        out.append((fr.copy(), fo.copy()))
    return out


@pytest.mark.parametrize("variant", list(__import__("oracle.ref_build", fromlist=["VARIANTS"]).VARIANTS))
@pytest.mark.parametrize("world_name", P.FRAME_WORLDS)
def test_frames(vxo, vxref, variant, world_name):
    dims = P.WORLDS[world_name][0]
    for cam in "ABCD":
        camera = P.frame_camera(cam, dims)
        pairs = _frame_pair(vxref, variant, world_name, camera, P.FRAME_W, P.FRAME_H, P.FRAME_NUMBERS)
        for n, (ref, got) in zip(P.FRAME_NUMBERS, pairs):
            bad = np.argwhere((ref != got).any(axis=2))
            assert bad.size == 0, "%s camera %s frame %d: %d pixels differ, first (y, x) %s: reference %s, oracle %s" % (
                variant, cam, n, len(bad), bad[0], ref[tuple(bad[0])], got[tuple(bad[0])])
        if vxref.switches(variant).get("checkerboard") and vxref.switches(variant).get("mode", 0) == 0:
            # the two parities together write every pixel but row 0 of the even columns (2 ty + 2 never is 0), which both
            # sides keep
            kept = (pairs[-1][0] == 77).all(axis=2)
            assert kept[0, 0::2].all() and not kept[1:].any() and not kept[0, 1::2].any()


_VARIANT_SWITCHES = {v: s for v, (_, _, s) in __import__("oracle.ref_build", fromlist=["VARIANTS"]).VARIANTS.items()}
_EXPRESSIBLE = [c for c in rec.CASES if P.variant_of_case(c, _VARIANT_SWITCHES) is not None]


def test_edge_cases_left_out():
    """the one render edge case the reference cannot run here: its world (65536 x 64 x 64) is above the 256^3 limit of
    reference-built worlds"""
    assert [c.name for c in rec.CASES if c not in _EXPRESSIBLE] == ["wide_long_axis"]


@pytest.mark.parametrize("case", _EXPRESSIBLE, ids=[c.name for c in _EXPRESSIBLE])
def test_render_edge_cases(vxo, vxref, case):
    """the frames are equal AND the case still reaches every branch it names (the oracle's census, as
    tests/test_render_edge_census.py asserts it on the cases' own worlds), over the two frame numbers together: a case that
    lost its target on the way here -- another world size, a variant's switches -- would compare nothing it was written for"""
    variants = _VARIANT_SWITCHES
    variant = P.variant_of_case(case, variants)
    assert rec.camera_rays_valid(case) and rec.light_valid(case.env["light_dir"])
    world_name = P.WORLD_OF_CASE[case.world]
    sw = variants[variant]
    r, w = P.reference_world(world_name, variant), P.oracle_world(world_name)
    W, H = case.W, case.H
    fr, fo = np.full((H, W, 4), 77, np.uint8), np.full((H, W, 4), 77, np.uint8)
    met = {t: 0 for t in case.targets}
    hits = 0
    for n in (case.frame_number, case.frame_number + 1):
        p = P.case_params(case, sw, n)
        out = w.render(p, fb=fo, want_census=True)
        cen = out["census"]
        assert not (cen & vxo.CEN_INVALID).any()
        for t in met:
            met[t] += int(((cen & getattr(vxo, "CEN_" + t)) != 0).sum())
        hits += out["stats"].primary_hits
        r.render(W, H, n, *P.case_camera(case), fb=fr, fov=case.fov, ortho_size=case.ortho_size, **case.env)
        bad = np.argwhere((fr != fo).any(axis=2))
        assert bad.size == 0, "%s (%s) frame %d: %d pixels differ, first (y, x) %s: reference %s, oracle %s" % (
            case.name, variant, n, len(bad), bad[0], fr[tuple(bad[0])], fo[tuple(bad[0])])
    assert all(met.values()) and hits > 0, (case.name, variant, met, hits)
