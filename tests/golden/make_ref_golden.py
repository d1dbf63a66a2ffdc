"""Generates tests/golden/ref_*.npz -- results RECORDED FROM THE REFERENCE'S OWN CODE, built as host C++ by
oracle/ref_build.py (needs the reference's sources on the machine; the fixtures themselves are used everywhere).

Unlike tests/golden/make_golden.py, whose vectors the oracle produced itself, these pin the oracle and the HIP path to the
reference: tests/test_ref_golden.py makes both reproduce them bit for bit, on any machine, without the reference.  The
inputs are rebuilt from seeds by tests/ref_pin_cases.py; each file carries a digest of its inputs.

    python tests/golden/make_ref_golden.py      # rewrites the fixtures (only when the reference snapshot or a definition changes)

Fixtures:
  ref_rays_<world>.npz     2048 mixed rays through random8, dense8 and random16: hit, steps, normal, position bits at
                           maxSteps 2048 and 8
  ref_builder.npz          the reference builder's coarse bits, extents and a SHA-256 per brick for one world per brick edge
                           (random8, random16, terrain32)
  ref_frames_<variant>.npz one 96x64 frame pair (FrameNumber 0 then 1 on one buffer) per reference variant: camera A over
                           the 256^3 terrain
  ref_meta.npz             the recipe's source hashes, the edits of every variant, flags and compiler (JSON); the 193 seeds
                           whose random float makes a bounce direction's x component exactly 0, found by running the
                           reference's function over all 2^32 seeds; and the result of the cast-sanitizer run

The cast-sanitizer run: every input of tests/test_reference_pin.py (rays at all four step budgets through the four worlds,
the same rays through the single-level traversal, the quirk cases, the ray / box cases, the builder worlds, the hash
seeds, the fBm points, the generator kernel, the frames of every variant and every expressible render edge case) goes once
through oracle/_ref/vxref_check_<variant> -- the driver plus oracle/ref_main.cpp, built with
-fsanitize=float-cast-overflow -fno-sanitize-recover, a stand-alone program on the CPU -- and must exit clean: no
float -> integer conversion of the reference receives a value outside its type.  The ten conversions that ref_build
routes through clamping conversions (CVT_I32, CVT_U32 there) are no casts any more: the sanitizer does not see them,
and at those ten points the reference's result is the clamp's definition, not its own.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import helpers, ref_pin_cases as P, render_edge_cases as rec  # noqa: E402

GOLDEN_CAMERA = "A"
GOLDEN_FRAME_WORLD = "terrain32"
STALE = 77                      # what the frame buffer holds before the first frame


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def brick_hashes(bricks) -> np.ndarray:
    """SHA-256 of every brick's words, (n, 32) uint8"""
    return np.array([np.frombuffer(hashlib.sha256(np.ascontiguousarray(b).tobytes()).digest(), np.uint8) for b in bricks], np.uint8)


def frame_params(variant_switches, frame_number):
    dims = P.WORLDS[GOLDEN_FRAME_WORLD][0]
    return P.make_params(P.FRAME_W, P.FRAME_H, P.frame_camera(GOLDEN_CAMERA, dims), variant_switches, frame_number)


def _variant_switches():
    from oracle import ref_build
    return {v: s for v, (_, _, s) in ref_build.VARIANTS.items()}


def _sanitizer_run(tmp):
    """every pin input through the cast-sanitized stand-alone programs; returns the lines they print"""
    from oracle import ref_build, vxo
    sw = _variant_switches()
    lines = []

    def run(variant, job):
        job.close()
        r = subprocess.run([os.path.join(ref_build.OUT, "vxref_check_" + variant), job.f.name], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("the cast sanitizer stopped vxref_check_%s:\n%s" % (variant, (r.stdout + r.stderr)[-2000:]))
        lines.append("%s: %s" % (variant, r.stdout.strip()))

    # traces, ray / box, hash, fBm: one program (the tracer and the noise code do not depend on the variant)
    for name in P.WORLDS:
        job = P.Job(os.path.join(tmp, "trace_%s.bin" % name))
        job.world(name)
        dims = P.WORLDS[name][0]
        f = P.WORLDS[name][1]
        w = P.oracle_world(name)
        for o, d in (P.adversarial_rays(dims), P.mixed_rays(dims)):
            for ms in P.MAX_STEPS:
                job.rays(o, d, ms)
                job.dda(P.dense(name), dims, o, d, ms)                                   # test_dda_single_level
                job.dda(w.coarse_bits, w.cdims, o / np.float32(f), d, ms, cell_boxes=w.bounds, scale=f)
        oa, da = P.adversarial_rays(dims)
        for ms in P.MAX_STEPS:
            for reg in (None, P.dda_region(dims)):
                for tis in (False, True):
                    if reg is not None or tis:
                        job.dda(P.dense(name), dims, oa, da, ms, region=reg, take_initial_step=tis)
        run("shadow_s1", job)
    job = P.Job(os.path.join(tmp, "small.bin"))
    for v, f, o, d, _ in P.quirk_inputs().values():
        job.world_dense(vxo.dense_from_voxels(v), *v.shape, f)
        w = vxo.World.from_voxels(v, f)
        o1, d1 = o.reshape(1, 3), d.reshape(1, 3)
        for ms in P.MAX_STEPS:
            job.rays(o1, d1, ms)
            job.dda(vxo.dense_from_voxels(v), v.shape, o1, d1, ms)                       # test_dda_quirk_cases
            job.dda(w.coarse_bits, w.cdims, o1 / np.float32(f), d1, ms, cell_boxes=w.bounds, scale=f)
            job.dda(vxo.dense_from_voxels(v), v.shape, o1, d1, ms, region=(0.0, 0.0, 0.0, float(v.shape[0] - f), float(v.shape[1]), float(v.shape[2])))
    for v, f in P.builder_worlds().values():                                            # test_builder
        job.world_dense(vxo.dense_from_voxels(v), *v.shape, f)
    job.populate(64, 64, 64)                                                            # test_populate_voxels
    job.aabb(*[np.concatenate([a, b]) for a, b in zip(P.aabb_cases(), P.quirk_aabb_cases())])
    job.seeds(P.hash_seeds())
    job.fbm(P.fbm_points())
    run("shadow_s1", job)
    # frames: each variant's own program
    for variant, s in sw.items():
        job = P.Job(os.path.join(tmp, "frames_%s.bin" % variant))
        for world_name in P.FRAME_WORLDS:
            job.world(world_name)
            for cam in "ABCD":
                camera = P.frame_camera(cam, P.WORLDS[world_name][0])
                for n in P.FRAME_NUMBERS:
                    job.frame(P.FRAME_W, P.FRAME_H, n, P.make_params(P.FRAME_W, P.FRAME_H, camera, s, n))
        for case in rec.CASES:
            if P.variant_of_case(case, sw) == variant:
                job.world(P.WORLD_OF_CASE[case.world])
                for n in (case.frame_number, case.frame_number + 1):
                    job.frame(case.W, case.H, n, P.case_params(case, s, n))
        run(variant, job)
    return lines


def _zero_x_seeds(vxref):
    out = []
    chunk = 1 << 26
    for base in range(0, 1 << 32, chunk):
        s = np.arange(base, base + chunk, dtype=np.uint64).astype(np.uint32)
        _, r = vxref.hash_and_random(s)
        out.append(s[(r * np.float32(2) - np.float32(1)) == 0])
    return np.concatenate(out).astype(np.uint32)


def main():
    from oracle import ref_build, vxref
    if not ref_build.build(verbose=True, sanitized=True):
        raise SystemExit("the reference's sources are needed to record fixtures from it")
    sw = _variant_switches()
    save = lambda name, **kw: np.savez_compressed(os.path.join(HERE, name + ".npz"), **kw)  # noqa: E731

    for name in P.GOLDEN_RAY_WORLDS:
        r = P.reference_world(name, vxref.DEFAULT)
        o, d = P.golden_rays(name)
        assert rec._valid(o, d).all()
        out = dict(inputs=digest(o, d, P.dense(name)))
        for ms in P.GOLDEN_MAX_STEPS:
            t = r.trace(o, d, ms)
            assert np.array_equal(t["normal"], t["normal"].astype(np.int8))
            out.update({"hit_%d" % ms: t["hit"], "steps_%d" % ms: t["steps"], "normal_%d" % ms: t["normal"].astype(np.int8),
                        "pos_bits_%d" % ms: helpers.float_bits(t["pos"])})
        save("ref_rays_" + name, **out)

    out = {}
    for f, name in P.GOLDEN_BUILDER_WORLDS.items():
        t = P.reference_world(name, vxref.DEFAULT).tables()
        occ = t["brick_dims"][:, 0] != 0
        out.update({name + "_inputs": digest(P.dense(name)), name + "_coarse_bits": t["coarse_bits"],
                    name + "_bounds": t["bounds"].astype(np.int8), name + "_brick_sha256": brick_hashes(t["bricks"][occ])})
        assert np.array_equal(t["bounds"], t["bounds"].astype(np.int8).astype(np.float32))
    save("ref_builder", **out)

    for variant, s in sw.items():
        r = P.reference_world(GOLDEN_FRAME_WORLD, variant)
        fbuf = np.full((P.FRAME_H, P.FRAME_W, 4), STALE, np.uint8)
        frames = []
        for n in P.FRAME_NUMBERS:
            p = frame_params(s, n)
            r.render(P.FRAME_W, P.FRAME_H, n, p.origin[:], p.fwd[:], p.up[:], p.right[:], fb=fbuf, fov=p.fov_deg,
                     ortho_size=p.ortho_size[:], light_dir=p.env.light_dir[:], light_color=p.env.light_color[:], ambient=p.env.ambient[:])
            frames.append(fbuf.copy())
        save("ref_frames_" + variant, inputs=digest(P.dense(GOLDEN_FRAME_WORLD), np.array(P.frame_camera(GOLDEN_CAMERA, (256, 256, 256))[0], np.float32)),
             switches=json.dumps(s, sort_keys=True), **{"fb_%d" % n: f for n, f in zip(P.FRAME_NUMBERS, frames)})

    with tempfile.TemporaryDirectory() as tmp:
        lines = _sanitizer_run(tmp)
    zero = _zero_x_seeds(vxref)
    assert len(zero) == 193, len(zero)
    save("ref_meta", manifest=json.dumps(ref_build.manifest(), sort_keys=True), zero_x_seeds=zero,
         sanitizer="-fsanitize=float-cast-overflow -fno-sanitize-recover: clean exit of every program\n" + "\n".join(lines))
    for f in sorted(os.listdir(HERE)):
        if f.startswith("ref_") and f.endswith(".npz"):
            print("%-32s %6d bytes" % (f, os.path.getsize(os.path.join(HERE, f))))


if __name__ == "__main__":
    main()
