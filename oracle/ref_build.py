"""Builds the REFERENCE's own sources as host C++ into oracle/_ref/ (test infrastructure; nothing of it is committed).

The reference is CUDA (.cu).  Its traversal, renderer, noise and world-builder code is plain C++ apart from three kernel
launch statements, so with a small shim (oracle/ref_shim.h: CUDA's header-only types, the launch coordinates as host
globals) and a driver (oracle/ref_driver.cpp: the runtime calls on the host heap and a C API) it compiles with a host
compiler and runs the reference's own arithmetic with IEEE binary32 semantics -- the definition the oracle claims to
restate.  tests/test_reference_pin.py compares the two bit for bit.

What the recipe does to the sources, all in temporary copies under oracle/_ref/src/ (EDITS below, by line number, with
text of our own; the committed repository holds no reference line):
  * the three kernel launch statements are dropped (the driver calls the kernels as functions, one thread at a time);
  * ten float -> integer conversions that ordinary inputs drive out of range (undefined in C++) are routed through
    ref_shim.h's clamping conversions, the behaviour of the reference's target (CVT_I32, CVT_U32 below);
  * per variant, the renderer's compile-time switches are set: the debug view define dropped, the checkerboard constant
    replaced by a -D macro, the commented-out shadow trace un-commented, the bounce sample count raised, ORTHO defined;
  * `#include "ref_driver.cpp"` is appended to the renderer copy, so that the driver sees the renderer's file-local frame
    record and switches.
The line numbers hold for one snapshot of the reference only, so every file the recipe reads is checked against a
recorded SHA-256 first and the build refuses a tree that differs.

Flags: the oracle's (-O2 -ffp-contract=off -fno-fast-math) plus -ftrivial-auto-var-init=zero, which makes the
reference's one uninitialised read (the step count the shading function adds up while the shadow trace is commented out;
it reaches no pixel) deterministic.  g++ before 12 does not know that flag; then the clang++ that ships with ROCm is used.

    python -m oracle.ref_build            # build every variant
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
REFERENCE_ROOT = os.environ.get("VXRT_REFERENCE_DIR", "/root/reference")
SUBDIR = "VoxelRT"

SHA256 = {
    "VolumeRaytracer.cu": "3686289344816b82215d9ba05ddd5df6cfec5fc20b9017e3a9e8f7ed1b75bb27",
    "VolumeRaytracer.cuh": "dd86fb6bfc764d168eeb59af1351bb67c38646d8a0977bd31c57334a72b46e3e",
    "Renderer.cu": "31e00a2bb6930c64401addbb9eb9b18a4107a2db9557b508d900487f88475e6e",
    "Renderer.cuh": "f847529808083c0107d17698753bd655eb8145ec411baad2700bff86f1d7275c",
    "VoxelWorldBuilder.cu": "2c96d1ea33237abe9c878d55131ec69b02d8fcc5474a8c4de7853aacdf8dacc2",
    "VoxelWorldBuilder.cuh": "1a7aa723cfd8d07a618cfd7d27a0425623668586e4741e4e21b7aab6e38a33f7",
    "cuda_noise.cu": "5a799cda6c8c849805d8b8773cf1be6ad28f239cbbb534b3a876f562127a4792",
    "cuda_noise.cuh": "420010a4d37205e1f4a5d11d35ef453244dd69b436456e6cd8b86511e6e736c6",
    "helper_math.h": "b0e5e1e20960dbf64891d9c1578b4c69872d926063eba4081a6ce9df3daee124",
}

# An edit: ("drop", first, last) removes lines first..last (1-based, inclusive); ("sub", line, regex, replacement)
# rewrites one line with re.sub and must change it; ("append", text) adds our own text at the end.
DROP_TRACE_LAUNCH = ("drop", 588, 590)          # VolumeRaytracer.cu: the batch kernel's launch statement
DROP_FRAME_LAUNCH = ("drop", 324, 325)          # Renderer.cu: the pixel kernel's launch statement
DROP_DEBUG_VIEW = ("drop", 4, 4)                # Renderer.cu: the debug view define
DROP_CHECKERBOARD = ("drop", 5, 5)              # Renderer.cu: the checkerboard constant (then given with -D ...=false)
ENABLE_SHADOW = ("sub", 102, r"false;\s*//\s*", "")   # Renderer.cu: un-comment the shadow trace behind `hit = false;//`
SAMPLES_1 = ("sub", 123, r"= 0;", "= 1;")       # Renderer.cu: bounce samples per pixel
SAMPLES_2 = ("sub", 123, r"= 0;", "= 2;")
DROP_POPULATE_LAUNCH = ("drop", 26, 26)         # VoxelWorldBuilder.cuh: the generator kernel's launch statement
# Conversions that ordinary inputs drive out of range (undefined in C++, clamping on the reference's target): the Perlin
# lattice hash takes a float beyond 2^32 in the higher octaves of EVERY point, and the tracer truncates positions that are
# infinite or NaN for rays with a denormal direction component.  They go through ref_shim.h's clamping conversions.
CVT_I32 = [("sub", n, r"static_cast<int>\(", "vxref_cvt_i32(") for n in (186, 187, 188, 441, 442, 443, 464, 465, 466)]   # VolumeRaytracer.cu
CVT_U32 = [("sub", 120, r"\(unsigned int\)", "vxref_cvt_u32")]                                                          # cuda_noise.cuh
APPEND_DRIVER = ("append", '\n#include "ref_driver.cpp"\n')
NO_CHECKERBOARD_DEFINE = "-DENABLE_CHECKERBOARD_RENDER=false"

# variant -> (edits of Renderer.cu before the common ones, extra -D flags, the oracle.vxo.make_params switches it equals)
VARIANTS = {
    "checked_in": ([], [], dict(mode=1, checkerboard=1)),
    "shaded": ([DROP_DEBUG_VIEW], [], dict(mode=0, checkerboard=1)),
    "shaded_nocb": ([DROP_DEBUG_VIEW, DROP_CHECKERBOARD], [NO_CHECKERBOARD_DEFINE], dict(mode=0, checkerboard=0)),
    "shadow_s1": ([DROP_DEBUG_VIEW, ENABLE_SHADOW, SAMPLES_1], [], dict(mode=0, checkerboard=1, shadow=1, bounce_samples=1)),
    "shadow_s2": ([DROP_DEBUG_VIEW, ENABLE_SHADOW, SAMPLES_2], [], dict(mode=0, checkerboard=1, shadow=1, bounce_samples=2)),
    # the two remaining combinations of the shadow trace and the bounce samples (render edge cases use them)
    "shaded_s1": ([DROP_DEBUG_VIEW, SAMPLES_1], [], dict(mode=0, checkerboard=1, shadow=0, bounce_samples=1)),
    "shadow_s0": ([DROP_DEBUG_VIEW, ENABLE_SHADOW], [], dict(mode=0, checkerboard=1, shadow=1, bounce_samples=0)),
    "ortho_shadow_s1": ([DROP_DEBUG_VIEW, ENABLE_SHADOW, SAMPLES_1], ["-DORTHO"],
                        dict(mode=0, checkerboard=1, shadow=1, bounce_samples=1, ortho=1)),
}
BASE_FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-ftrivial-auto-var-init=zero", "-fPIC", "-fpermissive", "-w"]
SANITIZE_FLAGS = ["-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


class ReferenceChanged(RuntimeError):
    pass


def reference_dir() -> str | None:
    d = os.path.join(REFERENCE_ROOT, SUBDIR)
    return d if os.path.isdir(d) else None


def lib_path(variant: str) -> str:
    return os.path.join(OUT, "libvxref_%s.so" % variant)


def check_path(variant: str) -> str:
    """the stand-alone cast-sanitized program of a variant (build(sanitized=True))"""
    return os.path.join(OUT, "vxref_check_" + variant)


RECIPE_FILES = ("ref_build.py", "ref_shim.h", "ref_driver.cpp")


def recipe_hash() -> str:
    """SHA-256 over the recipe's own files: libraries built from another state of them are stale"""
    h = hashlib.sha256()
    for name in RECIPE_FILES:
        with open(os.path.join(HERE, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def built() -> bool:
    """every variant's library is there and was built from the recipe as it stands now"""
    stamp = os.path.join(OUT, "recipe.sha256")
    if not all(os.path.exists(lib_path(v)) for v in VARIANTS) or not os.path.exists(stamp):
        return False
    with open(stamp) as f:
        return f.read().strip() == recipe_hash()


def check_snapshot(ref: str) -> None:
    for name, want in SHA256.items():
        path = os.path.join(ref, name)
        if not os.path.exists(path):
            raise ReferenceChanged("the reference has no %s: oracle/ref_build.py was written for another snapshot" % path)
        with open(path, "rb") as f:
            got = hashlib.sha256(f.read()).hexdigest()
        if got != want:
            raise ReferenceChanged("%s differs from the snapshot oracle/ref_build.py was written for (SHA-256 %s, recorded %s): "
                                   "its edits go by line number and would hit the wrong lines.  Review EDITS against the new "
                                   "text and record the new hashes." % (path, got, want))


def apply_edits(text: str, edits) -> str:
    lines = text.split("\n")
    tail = ""
    drop = set()
    for e in edits:
        if e[0] == "drop":
            drop.update(range(e[1], e[2] + 1))
        elif e[0] == "sub":
            new, n = re.subn(e[2], e[3], lines[e[1] - 1], count=1)
            if n != 1:
                raise ReferenceChanged("edit %r does not match line %d" % (e, e[1]))
            lines[e[1] - 1] = new
        elif e[0] == "append":
            tail += e[1]
        else:
            raise ValueError(e)
    return "\n".join("" if i + 1 in drop else l for i, l in enumerate(lines)) + tail     # dropped lines stay as blank lines


def cuda_include_dir() -> str:
    """A directory with CUDA's header-only runtime headers (cuda_runtime.h, vector_types.h, ...).  No CUDA toolkit or
    library is needed: only types and inline functions are used."""
    cands = [os.environ.get("VXRT_CUDA_INCLUDE")]
    spec = importlib.util.find_spec("triton")
    for loc in (spec.submodule_search_locations if spec else None) or []:
        cands.append(os.path.join(loc, "backends", "nvidia", "include"))
    cands += ["/usr/local/cuda/include"]
    for c in cands:
        if c and os.path.exists(os.path.join(c, "cuda_runtime.h")):
            return c
    raise RuntimeError("no CUDA runtime headers found (looked in VXRT_CUDA_INCLUDE, the triton package, /usr/local/cuda)")


def compiler() -> str:
    """g++ if it knows -ftrivial-auto-var-init (12 and later), otherwise ROCm's clang++"""
    cands = [os.environ.get("VXRT_REF_CXX"), "g++"]
    hipcc = shutil.which("hipcc")
    rocm = os.environ.get("ROCM_PATH", os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else "/opt/rocm")
    cands += [os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "clang++"]
    for c in cands:
        if not c or not shutil.which(c):
            continue
        r = subprocess.run([c, "-ftrivial-auto-var-init=zero", "-x", "c++", "-fsyntax-only", "-"], input=b"int x;\n",
                           capture_output=True)
        if r.returncode == 0:
            return c
    raise RuntimeError("no host compiler that knows -ftrivial-auto-var-init=zero (g++ >= 12 or clang++)")


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("reference build step failed: %s\n%s" % (" ".join(cmd), (r.stdout + r.stderr)[-4000:]))


def build(verbose: bool = False, sanitized: bool = False) -> bool:
    """Compile every variant into oracle/_ref/libvxref_<variant>.so.  Returns False, after one printed line and without
    touching an existing oracle/_ref/, where the reference's sources are not on this machine.  sanitized=True also links
    oracle/_ref/vxref_check_<variant>: the driver plus oracle/ref_main.cpp, built with -fsanitize=float-cast-overflow
    -fno-sanitize-recover (stand-alone programs; the sanitizer is never loaded into python)."""
    ref = reference_dir()
    if ref is None:
        print("oracle/ref_build: no reference sources at %s; oracle/_ref left as it is" % REFERENCE_ROOT)
        return False
    check_snapshot(ref)
    src, obj = os.path.join(OUT, "src"), os.path.join(OUT, "obj")
    os.makedirs(src, exist_ok=True)
    os.makedirs(obj, exist_ok=True)
    cxx = compiler()
    inc = cuda_include_dir()
    flags = BASE_FLAGS + ["-include", os.path.join(HERE, "ref_shim.h"), "-I" + src, "-I" + ref, "-I" + inc, "-I" + HERE]

    def read(name):
        with open(os.path.join(ref, name), encoding="utf-8", errors="surrogateescape") as f:
            return f.read()

    def write(name, text):
        with open(os.path.join(src, name), "w", encoding="utf-8", errors="surrogateescape") as f:
            f.write(text)

    write("vr_host.cpp", apply_edits(read("VolumeRaytracer.cu"), [DROP_TRACE_LAUNCH] + CVT_I32))
    write("cuda_noise.cuh", apply_edits(read("cuda_noise.cuh"), CVT_U32))                                # found before the reference's own
    write("VoxelWorldBuilder.cuh", apply_edits(read("VoxelWorldBuilder.cuh"), [DROP_POPULATE_LAUNCH]))   # found before the reference's own
    write("wb_host.cpp", read("VoxelWorldBuilder.cu"))
    write("noise_host.cpp", read("cuda_noise.cu"))
    for v, (edits, _, _) in VARIANTS.items():
        write("rn_%s.cpp" % v, apply_edits(read("Renderer.cu"), edits + [DROP_FRAME_LAUNCH, APPEND_DRIVER]))

    jobs = []           # (source, object, extra flags)
    for tag, extra in (("", []),) + ((("_san", SANITIZE_FLAGS),) if sanitized else ()):
        for s in ("vr_host", "wb_host", "noise_host"):
            jobs.append((s, s + tag, extra))
    for v, (_, defs, _) in VARIANTS.items():
        jobs.append(("rn_" + v, "rn_" + v, defs + ['-DVXREF_VARIANT="%s"' % v]))
    if sanitized:
        for v, (_, defs, _) in VARIANTS.items():
            jobs.append(("rn_" + v, "rn_%s_san" % v, defs + ['-DVXREF_VARIANT="%s"' % v] + SANITIZE_FLAGS))
        jobs.append((os.path.join(HERE, "ref_main"), "main_san", SANITIZE_FLAGS))

    def compile_one(job):
        s, o, extra = job
        _run([cxx] + flags + extra + ["-c", os.path.join(src, s + ".cpp"), "-o", os.path.join(obj, o + ".o")])     # (join keeps an absolute s)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(compile_one, jobs))
    shared = [os.path.join(obj, s + ".o") for s in ("vr_host", "wb_host", "noise_host")]
    for v in VARIANTS:
        tmp = lib_path(v) + ".tmp"
        _run([cxx, "-shared", "-Wl,-Bsymbolic", "-o", tmp, os.path.join(obj, "rn_%s.o" % v)] + shared + ["-lpthread", "-lm"])
        os.replace(tmp, lib_path(v))
    if sanitized:
        for v in VARIANTS:
            _run([cxx] + SANITIZE_FLAGS + ["-o", check_path(v), os.path.join(obj, "main_san.o"), os.path.join(obj, "rn_%s_san.o" % v)]
                 + [os.path.join(obj, s + "_san.o") for s in ("vr_host", "wb_host", "noise_host")] + ["-lpthread", "-lm"])
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest(version), f, indent=1, sort_keys=True)
    with open(os.path.join(OUT, "recipe.sha256"), "w") as f:
        f.write(recipe_hash() + "\n")
    if verbose:
        print("oracle/ref_build: %d reference variants built with %s" % (len(VARIANTS), version))
    return True


def manifest(compiler_version: str | None = None) -> dict:
    """what the libraries were built from: source hashes, the edits of each variant, flags and the compiler"""
    if compiler_version is None:
        with open(os.path.join(OUT, "manifest.json")) as f:
            return json.load(f)
    common = dict(trace=[DROP_TRACE_LAUNCH] + CVT_I32, noise_header=CVT_U32, world_builder_header=[DROP_POPULATE_LAUNCH], renderer_all=[DROP_FRAME_LAUNCH, APPEND_DRIVER])
    return dict(sha256=SHA256, common_edits=common, flags=BASE_FLAGS, compiler=compiler_version,
                variants={v: dict(renderer_edits=e, defines=d, switches=s) for v, (e, d, s) in VARIANTS.items()})


if __name__ == "__main__":
    sys.exit(0 if build(verbose=True, sanitized="--sanitized" in sys.argv) else 1)
