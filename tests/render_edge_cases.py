"""Render edge cases: frames whose inputs reach the branches the ordinary test cameras never do (helpers.CAMERAS are never
exactly axis-aligned, and they run with the default environment, FOV 90 and ortho sizes of 10 and more).

Every case names a world, an explicit binary32 camera (origin, fwd, up, right), FOV / ortho / ortho size, the environment,
the render options and the branches it is meant to reach, as oracle census bits (oracle/vxo.h VXO_CEN_*):
- the `special` rays of the tracer (vxrt_wave2.hpp: a direction component 0 or below 2^-40, or a start component -0.0) as
  primary, shadow and bounce rays: axis-aligned views, ortho views along an axis, axis-aligned lights, a camera origin of
  -0.0 on a world face, a tiny FOV, camera vectors with a 1e-30 or a subnormal component;
- the IEEE fall-backs of the render kernel's short division and square root (vxrt_device.hpp `ordinary`, exponent in
  [-100, 100]): camera vectors scaled by 1e-18 and 5e18 (squared ray length), a camera inside a solid voxel (view vector of
  length 0), light colours of 1e31, 1e38 and 1e-32 and a negative ambient that makes c + 1 exactly 0 (tonemap).
tests/test_render_edge_census.py proves on the oracle that each case reaches what it names and traces no invalid ray;
tests/test_gpu_render_edges.py compares the HIP frames of every case with the oracle bit for bit.

Two fall-backs no input reaches, with the evidence:
- The bounce direction.  Its squared length is not ordinary only when all three components random_float(s) * 2 - 1 are
  exactly 0: a component is a multiple of 2^-24 (or 0) in [-1, 1], so a non-zero one has a squared length of at least
  2^-48.  Enumerating all 2^32 seeds s with the oracle's vxo_random_float: 193 seeds give a zero x component, none of them
  also a zero y component (s * 10), so no seed -- and hence no frame_number, pixel or sample -- gives a zero direction.
- The view vector of a FAR camera (|hit - origin|^2 > 2^101, i.e. a camera more than 2^50.5 away).  Such a ray enters the
  grid at start + t * dir with t ~ 2^46 coarse cells or more: the entry point is rounded to a multiple of an ulp far wider
  than the grid, and the oracle finds no hit from y = 2^40, 2^60, 3e18 or 1e30 above a 512 x 256 x 512 terrain (axis-aligned
  rays down, on and off cell centres).  A near camera's view vector is 0 (camera inside a solid voxel) or at least the
  grid-entry epsilon (1e-6 coarse cells), never in (0, 2^-50).
  So the view-vector fall-back is reached only with a view vector of exactly 0 (the "inside" cases).  There the short
  square root gives NaN (v_rsq(0) = inf, 0 * inf) just as the IEEE operators do (1 / sqrt(0) = inf, 0 * inf), and the
  specular term is 0 either way: a build without that fall-back renders the same frames.  The cases still pin the
  branch's result; the tonemap fall-back, by contrast, changes pixels when removed (light_colour_1e38: c / (c + 1) with
  c + 1 above 2^126 has a subnormal reciprocal, which the short division loses).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import helpers

F32 = np.float32
INV3 = float(F32(1.0) / np.sqrt(F32(3.0)))
DEFAULT_ENV = dict(light_dir=(INV3, INV3, INV3), light_color=(2.0, 2.0, 2.0), ambient=(0.5, 0.5, 0.5))


@functools.lru_cache(maxsize=None)
def world(vxo, name):
    """the terrain floor (f = 32), random worlds at f = 16 and 8, a dense random world (density 0.6), the wide grid (8192
    coarse cells along x at f = 8)"""
    if name == "terrain32":
        return vxo.World.generate(vxo.GEN_INT_TERRAIN, 512, 256, 512, 32)
    if name == "random16":
        return helpers.random_voxel_world(vxo, (128, 128, 128), 16, 0.004, 41)
    if name == "random8":
        return helpers.random_voxel_world(vxo, (64, 64, 64), 8, 0.03, 42)
    if name == "dense8":
        v = np.random.default_rng(43).random((64, 64, 64)) < 0.6
        v[28:36, 28:36, 28:36] = True            # the camera of the "inside" case sits in this solid block
        return vxo.World.from_voxels(v, 8)
    if name == "wide8":
        X = 8192 * 8
        rng = np.random.default_rng(8192)
        v = np.zeros((X, 64, 64), bool)
        n_vox = int(X * 64 * 64 * 0.000004)
        v[rng.integers(0, X, n_vox), rng.integers(0, 64, n_vox), rng.integers(0, 64, n_vox)] = True
        v[:, 0, :] = True
        return vxo.World.from_voxels(v, 8)
    raise KeyError(name)


def _v(x):
    return tuple(float(F32(c)) for c in x)


def _unit(x):
    a = np.asarray(x, np.float64)
    return _v(a / np.linalg.norm(a))


def _euler(euler):
    """GetDirections (Renderer.cu:27-42) in binary32, as the host library and the oracle compute it"""
    e = np.asarray(euler, np.float32)
    fx, fy, fz = np.cos(e[0]) * np.sin(e[1]), -np.sin(e[0]), np.cos(e[0]) * np.cos(e[1])
    rx, ry, rz = np.cos(e[1]), F32(0), -np.sin(e[1])
    ux, uy, uz = fy * rz - fz * ry, fz * rx - fx * rz, fx * ry - fy * rx
    return _v((fx * F32(-1), fy * F32(-1), fz * F32(-1))), _v((ux * F32(-1), uy * F32(-1), uz * F32(-1))), _v((rx, ry, rz))


CAM_A_EULER = helpers.CAMERAS["A"][1]


class Case:
    def __init__(self, name, world, targets, pos, fwd, up, right, *, W=64, H=48, fov=90.0, ortho=0, ortho_size=(10.0, 10.0),
                 env=None, frame_number=3, **opts):
        self.name, self.world, self.targets = name, world, tuple(targets)
        self.W, self.H = W, H
        self.camera = (_v(pos), _v(fwd), _v(up), _v(right))
        self.fov, self.ortho, self.ortho_size = float(F32(fov)), ortho, _v(ortho_size)
        self.env = dict(DEFAULT_ENV, **(env or {}))
        self.env = {k: _v(v) for k, v in self.env.items()}
        self.frame_number = frame_number
        self.opts = dict(dict(shadow=1, bounce_samples=1), **opts)

    def render_kw(self):
        """keyword arguments of oracle.vxo.make_params (and of test_gpu_parity._render_both) after W, H and the camera"""
        return dict(fov=self.fov, ortho=self.ortho, ortho_size=self.ortho_size, frame_number=self.frame_number,
                    **self.env, **self.opts)

    def params(self, vxo):
        return vxo.make_params(self.W, self.H, *self.camera, **self.render_kw())

    def __repr__(self):
        return "Case(%s)" % self.name


X_, Y_, Z_ = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
NX, NY, NZ = (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)
SP, SS = "SPECIAL_PRIMARY", "SPECIAL_SHADOW"
F0, U0, R0 = _euler((0.0, 0.0, 0.0))                            # fwd (-0, 0, -1), right (1, 0, -0)
FP, UP, RP = _euler((0.0, float(F32(np.pi / 2)), 0.0))
FM, UM, RM = _euler((0.0, float(F32(-np.pi / 2)), 0.0))
FA, UA, RA = _euler(CAM_A_EULER)
POS_A = (256.0, 230.0, 256.0)                                   # camera A over the 512 x 256 x 512 terrain, lower down

CASES = [
    # ---- axis-aligned views (even W and H: the centre column and row are exactly 0 along one axis)
    Case("opening_view", "terrain32", (SP,), (256, 256, 256), Z_, Y_, X_),   # VoxelApp/main.cu's first frame
    Case("view_px", "terrain32", (SP,), (8, 150, 256), X_, Y_, NZ, bounce_depth=2),
    Case("view_nx", "terrain32", (SP,), (504, 150, 256), NX, Y_, Z_),
    Case("view_ny_topdown", "terrain32", (SP,), (256, 300, 256), NY, Z_, X_, bounce_depth=2, bounce_all_hits=1),
    Case("view_py_from_below", "terrain32", (SP,), (256, -20, 256), Y_, Z_, X_),
    Case("view_nz", "terrain32", (SP,), (256, 180, 504), NZ, Y_, X_, checkerboard=1),
    Case("view_pz_debug", "random16", (SP,), (64, 64, -10), Z_, Y_, X_, mode=1),
    Case("euler_zero", "terrain32", (SP,), (256, 180, 400), F0, U0, R0),
    Case("euler_plus_half_pi", "terrain32", (SP,), (450, 180, 256), FP, UP, RP),
    Case("euler_minus_half_pi", "terrain32", (SP,), (60, 180, 256), FM, UM, RM, bounce_samples=2),
    Case("neg_zero_origin_axis", "random8", (SP,), (-0.0, 32, 32), X_, Y_, NZ),
    Case("neg_zero_origin_oblique", "random8", (SP,), (-0.0, 40, 20), _unit((1, -0.3, 0.4)), _unit((0.3, 1, 0)),
         _unit((-0.4, 0, 1))),
    Case("wide_long_axis", "wide8", (SP,), (8, 30, 32), X_, Y_, NZ),
    # ---- ortho along an axis: W = H = 64 and size 32 put the pixel origins on integer grid lines (cell and brick faces)
    Case("ortho_topdown_grid_lines", "terrain32", (SP, SS), (256, 300, 256), NY, Z_, X_, W=64, H=64, ortho=1,
         ortho_size=(32, 32), env=dict(light_dir=Y_), bounce_depth=2),
    Case("ortho_px_grid_lines", "random8", (SP,), (-5, 32, 32), X_, Y_, Z_, W=64, H=64, ortho=1, ortho_size=(32, 32)),
    Case("ortho_size_zero", "terrain32", (SP,), (200, 300, 300), NY, Z_, X_, ortho=1, ortho_size=(0, 0)),
    Case("ortho_size_negative", "terrain32", (SP,), (300, 300, 200), NY, Z_, X_, ortho=1, ortho_size=(-10, -10)),
    # ---- lights: shadow rays along an axis, with a zero or tiny component, a light that is not of unit length
    Case("light_py", "terrain32", (SS,), POS_A, FA, UA, RA, env=dict(light_dir=Y_), bounce_depth=2, bounce_all_hits=1),
    Case("light_px", "terrain32", (SS,), POS_A, FA, UA, RA, env=dict(light_dir=X_), bounce_depth=2),
    Case("light_nz", "terrain32", (SS,), POS_A, FA, UA, RA, env=dict(light_dir=NZ)),
    Case("light_one_zero", "terrain32", (SS,), POS_A, FA, UA, RA, env=dict(light_dir=(0.6, 0.8, 0.0))),
    Case("light_not_unit", "terrain32", (SS,), POS_A, FA, UA, RA, env=dict(light_dir=(3.0, 4.0, 0.0))),
    Case("light_tiny_component", "terrain32", (SS,), POS_A, FA, UA, RA, env=dict(light_dir=(0.6, 0.8, 1e-13))),
    Case("light_axis_view_axis", "terrain32", (SP, SS), (256, 180, 400), NZ, Y_, X_, env=dict(light_dir=X_),
         bounce_depth=2),
    # ---- FOV
    Case("fov_tiny", "terrain32", (SP,), (256, 180, 400), NZ, Y_, X_, fov=1e-10),
    Case("fov_1", "terrain32", (SP,), (256, 180, 400), NZ, Y_, X_, fov=1.0),
    Case("fov_30", "terrain32", (SP,), (256, 180, 400), NZ, Y_, X_, fov=30.0),
    Case("fov_170", "terrain32", (SP,), (256, 180, 400), NZ, Y_, X_, fov=170.0),
    # ---- camera vectors not of unit length; a fwd with a tiny or subnormal component
    Case("camera_scale_1e-18", "terrain32", ("CAM_LEN",), POS_A, *[tuple(F32(c) * F32(1e-18) for c in v) for v in (FA, UA, RA)]),
    Case("camera_scale_5e18", "terrain32", ("CAM_LEN",), POS_A, *[tuple(F32(c) * F32(5e18) for c in v) for v in (FA, UA, RA)]),
    Case("fwd_component_1e-30", "terrain32", (SP,), (256, 180, 400), (1e-30, 0.0, -1.0), Y_, X_),
    Case("fwd_component_subnormal", "terrain32", (SP,), (256, 180, 400), (1e-40, 0.0, -1.0), Y_, X_),
    # ---- a camera inside a solid voxel: the view vector has length 0 (no shadow ray: it would start inside the voxel)
    Case("inside_dense", "dense8", ("VIEW",), (31.5, 31.5, 31.5), FA, UA, RA, shadow=0),
    Case("inside_terrain", "terrain32", ("VIEW",), (256.5, 20.5, 256.5), NY, Z_, X_, shadow=0, bounce_samples=0),
    # ---- colours far from 1
    Case("light_colour_1e31", "terrain32", ("TONEMAP",), POS_A, FA, UA, RA, env=dict(light_color=(1e31, 1e31, 1e31))),
    Case("light_colour_1e38", "terrain32", ("TONEMAP",), POS_A, FA, UA, RA, env=dict(light_color=(1e38, 2e38, 3e38))),
    Case("light_colour_1e-32_ambient_0", "terrain32", ("TONEMAP",), POS_A, FA, UA, RA,
         env=dict(light_color=(1e-32, 1e-32, 1e-32), ambient=(0, 0, 0))),
    Case("ambient_minus_one", "terrain32", ("TONEMAP",), POS_A, FA, UA, RA, env=dict(ambient=(-1, -1, -1)), bounce_samples=0),
    Case("colour_zero", "terrain32", (SS,), POS_A, FA, UA, RA, env=dict(light_dir=Y_, light_color=(0, 0, 0), ambient=(0, 0, 0))),
]
CASE_IDS = [c.name for c in CASES]


# ---- ray validity on the host (include/vxrt.h: finite origin, squared direction length positive and finite, binary32)
def _valid(o, d):
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        osum = np.abs(o[..., 0]) + np.abs(o[..., 1]) + np.abs(o[..., 2])
        dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    return np.isfinite(osum) & (dd > 0) & np.isfinite(dd)


def camera_rays(case):
    """getRayDirection / getRayDirectionOrtho (Renderer.cu:44-70, vxrt_persist2.hpp camera_ray) restated in binary32 numpy
    over every pixel: (origins, directions) of shape (H, W, 3), the directions before normalisation; with case.rows = (y0, y1)
    over the rows y0 .. y1 - 1 of the frame alone"""
    W, H = case.W, case.H
    pos, fwd, up, right = (np.asarray(v, np.float32) for v in case.camera)
    y0, y1 = getattr(case, "rows", None) or (0, H)
    y, x = np.mgrid[y0:y1, 0:W]
    u = x.astype(np.float32) / F32(W)
    v = y.astype(np.float32) / F32(H)
    su, sv = (u * F32(2) - F32(1))[..., None], (v * F32(2) - F32(1))[..., None]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if case.ortho:
            ratio = F32(W) / F32(H)
            o = pos + ((right * su) * F32(case.ortho_size[0])) * ratio
            o = o + (up * sv) * F32(case.ortho_size[1])
            d = np.broadcast_to(fwd, o.shape)
        else:
            aspect = F32(W) / F32(H)
            fov = F32(float(case.fov) * 3.1415 / 180.0)
            ky = np.tan(fov / F32(2), dtype=np.float32)
            kx = ky * aspect
            d = fwd + su * kx * right + sv * ky * up
            o = np.broadcast_to(pos, d.shape)
    return o, d


def camera_rays_valid(case):
    o, d = camera_rays(case)
    return bool(_valid(o, d).all())


def light_valid(light_dir):
    """the shadow ray's direction unit3(L) (vxrt_api.hip, on the host) is a valid direction"""
    L = np.asarray(light_dir, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        dd = L[0] * L[0] + L[1] * L[1] + L[2] * L[2]
        unit = L * (F32(1) / np.sqrt(dd, dtype=np.float32))
    return bool(_valid(np.zeros(3, np.float32), unit)) and bool(np.isfinite(unit).all())


# ---- random edge-case frames for tests/tools/fuzz_parity.py
AXES = [X_, Y_, Z_, NX, NY, NZ]


def random_axis_camera(rng, dims):
    """a random axis-aligned view of a world of `dims`: fwd along an axis, up and right along the other two (either sign),
    the origin inside the grid, on a face (0 or -0.0 included) or outside it, on integer coordinates half of the time"""
    a = int(rng.integers(0, 6))
    fwd = AXES[a]
    others = [b for b in range(3) if b != a % 3]
    up, right = [0.0] * 3, [0.0] * 3
    up[others[0]] = float(rng.choice([-1.0, 1.0]))
    right[others[1]] = float(rng.choice([-1.0, 1.0]))
    if rng.random() < 0.5:
        up, right = right, up
    pos = [float(rng.uniform(-0.2, 1.2) * d) for d in dims]
    if rng.random() < 0.5:
        pos = [float(np.floor(p)) for p in pos]
    k = int(rng.integers(0, 3))
    if rng.random() < 0.3:
        pos[k] = -0.0 if rng.random() < 0.5 else float(dims[k])
    return tuple(pos), fwd, tuple(up), tuple(right)


def random_environment(rng):
    """light direction (an axis, one zero component, not of unit length, or the default), light colour and ambient (far
    from 1, zero, or negative with c + 1 = 0 on lit-from-above faces), FOV"""
    k = int(rng.integers(0, 5))
    if k == 0:
        light = AXES[int(rng.integers(0, 6))]
    elif k == 1:
        light = (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), 0.0)
    elif k == 2:
        light = (3.0, 4.0, float(rng.choice([0.0, 1e-13, 2.0])))
    else:
        light = DEFAULT_ENV["light_dir"]
    colour = float(rng.choice([2.0, 0.0, 1e-32, 1e31, 1e38]))
    ambient = float(rng.choice([0.5, 0.0, -1.0, 1e-32]))
    fov = float(rng.choice([90.0, 1e-10, 1.0, 30.0, 170.0]))
    return dict(light_dir=_v(light), light_color=(colour,) * 3, ambient=(ambient,) * 3), fov
