"""The cases of the sky-on-frames tests (include/vxrt.h, vxrt_sky_frame), shared by the host and the GPU tests: random cases
that are functions of their arguments alone, and hand-derived cases of one pixel under an ortho camera, whose ray is the
camera's forward vector as it is, with dyadic parameters, so that every expected number can be written out."""
import numpy as np

from tests import ref_denoise as R
from tests import ref_sky as SK

F32 = np.float32
WORLD = (4096, 4096, 4096)  # what the random keys are made for: no world is resident in these tests
ORTHO_SIZE = (24.0, 20.0)
# the frames of the contract's tests: they straddle a wave's 64 lanes and a workgroup's 4 rows
FRAMES = ((1, 1), (63, 5), (64, 4), (65, 3), (130, 9), (257, 2))
# (W, H, ortho, pose)
CASES = ([(W, H, ortho, "level") for W, H in FRAMES for ortho in (False, True)] +
         [(130, 9, False, "up"), (130, 9, True, "up"), (130, 9, False, "down"), (65, 3, False, "high"), (64, 4, True, "axis"), (67, 35, False, "level"),
          (65, 5, False, "level")])  # partial tiles on both axes
POSES = {  # origin, fwd, up, right
    "level": ((100.5, 60.25, 80.75), (0.8, 0.1, 0.6), (0.05, 0.99, -0.1), (0.6, 0.0, -0.8)),
    "up": ((100.5, 60.25, 80.75), (0.3, 0.9, 0.3), (0.6, -0.4, 0.6), (0.7, 0.0, -0.7)),
    "down": ((100.5, 160.25, 80.75), (0.2, -0.9, 0.3), (0.3, 0.3, 0.9), (0.95, 0.1, -0.3)),
    "high": ((100.5, 460.25, 80.75), (0.8, 0.3, 0.5), (0.0, 1.0, 0.0), (0.5, 0.0, -0.8)),  # above the cloud plane
    # an ortho ray with d.z == 0 and a denormal d.x: keys of axis 2 are copied for d[a] == 0, keys of axis 0 for an infinite t
    "axis": ((100.5, 60.25, 80.75), (1e-39, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),
}
# what the random cases run under: every glow_log2, octaves 1 and 6, with and without clouds
PARAM_SETS = [dict(flags=SK.CLOUDS, glow_log2=g, octaves=o) for g, o in ((0, 1), (1, 6), (2, 3), (3, 6), (4, 1), (5, 2), (6, 6), (7, 4), (8, 5))] + [
    dict(flags=0, glow_log2=3, octaves=4)]


def random_params(rng, pose):
    """a sky whose sun stands near the camera's forward vector (with a wide disc, so that a small frame shows it), a cloud
    plane at y = 300 and fog that starts inside the range of the hit distances"""
    fwd = np.asarray(POSES[pose][1], np.float64)
    sun = fwd + rng.uniform(-0.1, 0.1, 3)
    sun[1] = abs(sun[1]) + 0.05
    col = lambda lo, hi: tuple(float(F32(v)) for v in rng.uniform(lo, hi, 3))
    return dict(zenith=col(0.0, 0.5), horizon=col(0.5, 1.0), ground=col(0.1, 0.4), sun_color=col(0.7, 1.2), cloud_color=col(0.8, 1.0),
                sun_dir=tuple(float(v) for v in sun * rng.uniform(0.5, 3.0)), glow_strength=float(rng.uniform(0.1, 0.6)),
                ground_fade=float(rng.uniform(1.0, 6.0)), cos_inner=0.98, cos_outer=0.9, cloud_y=300.0, cloud_scale=float(rng.uniform(0.002, 0.02)),
                cloud_offset=(float(rng.uniform(-50, 50)), float(rng.uniform(-50, 50))), cloud_max_t=2000.0, cloud_cover=float(rng.uniform(0.4, 0.7)),
                cloud_sharp=float(rng.uniform(2.0, 8.0)), cloud_fade=float(rng.uniform(2.0, 10.0)), fog_start=float(rng.uniform(10.0, 40.0)),
                fog_density=float(rng.uniform(0.005, 0.05)), fog_max=float(rng.uniform(0.5, 0.9)), seed=int(rng.integers(0, 1 << 32)))


def random_case(W, H, ortho, pose="level", seed=0):
    """colours from tests/ref_denoise.py's random frames with NaNs sprinkled in; keys of five kinds: misses, faces of voxels on
    the pixel's own ray at 2 .. 300 voxels, the same with the axis field raised above 2, faces far behind or ahead of the
    camera (random plane, axis and side), and the plane 2^25 - 1.  Everything read-only."""
    rng = np.random.default_rng(7919 * W + 31 * H + 5 * seed + int(ortho) + 11 * sorted(POSES).index(pose))
    cam = tuple(np.asarray(v, F32) for v in POSES[pose])
    o, d = R.primary_rays(W, H, *cam, ortho=ortho, ortho_size=ORTHO_SIZE)
    color, _ = R.random_frame(W, H, seed)
    color = color.copy()
    color[rng.random((H, W)) < 0.03] = F32(np.nan)
    X, Y, Z = WORLD
    with np.errstate(invalid="ignore", over="ignore"):
        along = np.nan_to_num(o.astype(np.float64) + rng.uniform(2.0, 300.0, (H, W, 1)) * d, nan=0.0, posinf=0.0, neginf=0.0)
    along = np.clip(along.astype(np.int64), 0, np.array(WORLD) - 1)
    hit = along[..., 0] + X * (along[..., 1] + Y * along[..., 2])
    keys = R.keys_np(hit, WORLD, o, d).astype(np.uint32)
    pick = rng.random((H, W))
    raised = keys | (rng.integers(1, 8, (H, W)).astype(np.uint32) << np.uint32(28))  # an axis field of 16 .. 127 & 31: above 2
    anyface = (np.uint32(1 << 31) | (rng.integers(0, 3, (H, W)).astype(np.uint32) << np.uint32(26)) |
               (rng.integers(0, 2, (H, W)).astype(np.uint32) << np.uint32(25)) | rng.integers(0, 4096, (H, W)).astype(np.uint32))
    keys = np.where(pick < 0.35, np.uint32(0), keys)
    keys = np.where((pick >= 0.75) & (pick < 0.8), raised, keys)
    keys = np.where((pick >= 0.8) & (pick < 0.95), anyface, keys)
    keys = np.where(pick >= 0.95, anyface | np.uint32(0x1FFFFFF), keys).astype(np.uint32)
    for a in (color, keys):
        a.setflags(write=False)
    return dict(color=color, keys=keys, cam=cam, ortho=ortho, ortho_size=ORTHO_SIZE, params=random_params(rng, pose))


def run_case(case, p=None, scalar=False, pixels=None):
    kw = {}
    color, keys = case["color"], case["keys"]
    if pixels is not None:
        H, W = keys.shape
        pixels = np.asarray(pixels).reshape(-1, 2)
        kw = dict(pixels=pixels, dims=(W, H))
        color, keys = color[pixels[:, 1], pixels[:, 0]], keys[pixels[:, 1], pixels[:, 0]]
    return SK.sky_frame(color, keys, case["cam"], dict(case["params"], **(p or {})), case["ortho"], ortho_size=case["ortho_size"],
                        scalar=scalar, **kw)


# ---- hand-derived cases ------------------------------------------------------------------------------------------------
# One pixel under an ortho camera: W = H = 1, window (1, 1), right = +x, up = +z, so the ray starts at
# pos + ((right * -1) * 1) * 1 + (up * -1) * 1 = pos - (1, 0, 1) and its direction is fwd as it is (not normalised).
HAND = dict(flags=0, glow_log2=1, octaves=2, seed=7, zenith=(0.25, 0.5, 1.0), horizon=(0.75, 0.75, 0.75), ground=(0.25, 0.25, 0.125),
            sun_color=(1.0, 0.5, 0.25), cloud_color=(1.0, 1.0, 1.0), sun_dir=(0.0, 0.0, 2.0), glow_strength=0.5, ground_fade=2.0,
            cos_inner=0.75, cos_outer=0.5, cloud_y=100.0, cloud_scale=0.25, cloud_offset=(0.5, 0.25), cloud_max_t=1000.0, cloud_cover=0.5,
            cloud_sharp=4.0, cloud_fade=1.0, fog_start=4.0, fog_density=0.25, fog_max=0.5)
WINDOW = (1.0, 1.0)


def key(axis_field, toward, plane):
    return 0x80000000 | (axis_field << 26) | (toward << 25) | plane


def one_pixel(o, d, k=0, color=(0.5, 0.5, 0.5), **p):
    """the case of one pixel with ray (o, d), key k and input colour `color` under HAND overridden by p"""
    cam = ((o[0] + 1.0, o[1], o[2] + 1.0), d, (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    return dict(color=np.array([[color]], F32), keys=np.array([[k]], np.uint32), cam=tuple(np.asarray(v, F32) for v in cam), ortho=True,
                ortho_size=WINDOW, params=dict(HAND, **p))


def zenith():
    """d = (0, 1, 0): h = 1, a = 0, a4 = 0: zenith + (horizon - zenith) * 0 = zenith.  s = (0, 0, 2) / 2 = (0, 0, 1), sd = 0: g = 0,
    + sun_color * (0.5 * 0) adds 0.  e = smooth(clamp01((0 - 0.5) / 0.25 = -2)) = 0: c + (sun_color - c) * 0 = c.  No clouds."""
    return one_pixel((8.0, 16.0, 8.0), (0.0, 1.0, 0.0)), [0.25, 0.5, 1.0], (1, 0, 0, 0, 0, 0)


def horizon_with_glow():
    """d = (0.5, 0, 0.5): h = 0, a4 = 1: zenith + (horizon - zenith) * 1 = 0.25 + 0.5, 0.5 + 0.25, 1.0 - 0.25 = 0.75 each.
    sd = 0.5, squared once (glow_log2 = 1): g = 0.25, k = 0.5 * 0.25 = 0.125: c = 0.75 + (1, 0.5, 0.25) * 0.125.
    e = smooth(clamp01((0.5 - 0.5) / 0.25)) = 0: no disc.  h = 0 is no ground."""
    return one_pixel((8.0, 16.0, 8.0), (0.5, 0.0, 0.5)), [0.875, 0.8125, 0.78125], (1, 0, 0, 0, 0, 0)


def straight_at_the_sun():
    """d = s = (0, 0, 1): h = 0, sd = 1: base = 0.75 + sun_color * 0.5 = (1.25, 1.0, 0.875).  e = smooth(clamp01((1 - 0.5) / 0.25 = 2)
    = 1) = (1 * 1) * (3 - 2) = 1: c + (sun_color - c) * 1 = 1.25 - 0.25, 1.0 - 0.5, 0.875 - 0.625 = sun_color."""
    return one_pixel((8.0, 16.0, 8.0), (0.0, 0.0, 1.0)), [1.0, 0.5, 0.25], (1, 0, 0, 1, 0, 0)


def ground(dy=-1.0):
    """d = (0, -1, 0): (-h) * ground_fade = 2, clamped to 1 (dy = -0.5: exactly 1): horizon + (ground - horizon) * 1 =
    0.75 - 0.5, 0.75 - 0.5, 0.75 - 0.625 = ground.  No glow, no disc, no clouds below the horizon."""
    return one_pixel((8.0, 16.0, 8.0), (0.0, dy, 0.0)), [0.25, 0.25, 0.125], (1, 0, 1, 0, 0, 0)


def hit_before_the_fog():
    """o.y = 10, d = (0, -1, 0), the face y = 6 seen from above: t = (6 - 10) / -1 = 4 = fog_start: u = 0, x = 0, f = 0: copied"""
    return one_pixel((8.0, 10.0, 8.0), (0.0, -1.0, 0.0), key(1, 0, 6), (0.5, -0.0, 3.0)), [0.5, -0.0, 3.0], (0, 1, 0, 0, 0, 0)


def hit_in_the_fog():
    """o.y = 14, the face y = 6: t = 8, u = 4, x = 4 * 0.25 = 1, f = 1 / 2 = 0.5 (fog_max 0.75 is not reached).  base(d) = ground:
    out = 0.5 + (ground - 0.5) * 0.5 = 0.5 - 0.125, 0.5 - 0.125, 0.5 - 0.1875"""
    return one_pixel((8.0, 14.0, 8.0), (0.0, -1.0, 0.0), key(1, 0, 6), fog_max=0.75), [0.375, 0.375, 0.3125], (0, 1, 0, 0, 0, 1)


def hit_far_away():
    """o.y = 1028, the face y = 0: t = 1028, u = 1024, x = 256, f = 256 / 257 > fog_max = 0.5: f = 0.5, the same colour as at t = 8"""
    return one_pixel((8.0, 1028.0, 8.0), (0.0, -1.0, 0.0), key(1, 0, 0)), [0.375, 0.375, 0.3125], (0, 1, 0, 0, 0, 1)


def hit_without_fog():
    """fog_density = 0: x = 0 at every distance: the colour is copied bit for bit -- -0 stays -0 and an infinity stays one"""
    return (one_pixel((8.0, 1028.0, 8.0), (0.0, -1.0, 0.0), key(1, 0, 0), (-0.0, np.inf, 1e30), fog_density=0.0), [-0.0, np.inf, 1e30],
            (0, 1, 0, 0, 0, 0))


def hit_with_axis_field_3():
    """an axis field of 3 reads as axis 2: d = (0, 0, 1), o.z = 2, plane 10: t = 8 as in hit_in_the_fog; base(d) is the sky straight
    at the sun without its disc, (1.25, 1.0, 0.875): out = 0.5 + (base - 0.5) * 0.5 = 0.875, 0.75, 0.6875"""
    return one_pixel((8.0, 16.0, 2.0), (0.0, 0.0, 1.0), key(3, 1, 10), fog_max=0.75), [0.875, 0.75, 0.6875], (0, 1, 0, 0, 0, 1)


def hit_along_the_face():
    """d = (0, 0, 1) and a key of axis 0: d[a] == 0: copied"""
    return one_pixel((8.0, 16.0, 2.0), (0.0, 0.0, 1.0), key(0, 1, 100)), [0.5, 0.5, 0.5], (0, 1, 0, 0, 0, 0)


def hit_behind_the_camera():
    """o.y = 10, d = (0, -1, 0), the plane y = 20: t = (20 - 10) / -1 = -10 < 0: copied"""
    return one_pixel((8.0, 10.0, 8.0), (0.0, -1.0, 0.0), key(1, 0, 20)), [0.5, 0.5, 0.5], (0, 1, 0, 0, 0, 0)


def nan_on_a_hit():
    """a NaN input colour in the fog: c + (base - c) * f stays NaN"""
    return one_pixel((8.0, 14.0, 8.0), (0.0, -1.0, 0.0), key(1, 0, 6), (np.nan, 0.5, np.nan)), [np.nan, 0.375, np.nan], (0, 1, 0, 0, 0, 1)


def nan_on_a_miss():
    """a miss pixel's input colour is not looked at: the zenith case with NaN in"""
    return one_pixel((8.0, 16.0, 8.0), (0.0, 1.0, 0.0), 0, (np.nan, np.nan, np.nan)), [0.25, 0.5, 1.0], (1, 0, 0, 0, 0, 0)


def camera_above_the_clouds():
    """o.y = 116 > cloud_y = 100 under VXRT_SKY_CLOUDS: no cloud: the zenith colour"""
    return one_pixel((8.0, 116.0, 8.0), (0.0, 1.0, 0.0), flags=SK.CLOUDS), [0.25, 0.5, 1.0], (1, 0, 0, 0, 0, 0)


def cloud_coordinate_out_of_range():
    """cloud_scale = 2^28, o.x = 8: px = (8 + 84 * 0) * 2^28 + 0.5 = 2^31, px * 2^(octaves - 1) = 2^32 >= 2^30: no cloud"""
    return one_pixel((8.0, 16.0, 8.0), (0.0, 1.0, 0.0), flags=SK.CLOUDS, cloud_scale=2.0 ** 28), [0.25, 0.5, 1.0], (1, 0, 0, 0, 0, 0)


def no_cloud_cover():
    """cloud_cover = 0: n < 1 always (the values stay below 1 and the octave weights add up to less than 1), n - 1 < 0: dens = 0,
    alpha = 0: c + (cloud_color - c) * 0 = c: the zenith colour, and `cloud` is not counted"""
    return one_pixel((8.0, 16.0, 8.0), (0.0, 1.0, 0.0), flags=SK.CLOUDS, cloud_cover=0.0), [0.25, 0.5, 1.0], (1, 0, 0, 0, 0, 0)


def full_cloud_cover():
    """cloud_cover = 1, cloud_sharp = 2^20: dens = clamp01(n * 2^20) = 1 for every n >= 2^-20 (n is a sum of multiples of 2^-25
    times weights: smaller only by accident, and not at this point); h = 1, cloud_fade = 1: alpha = 1:
    c + (cloud_color - c) * 1 = 0.25 + 0.75, 0.5 + 0.5, 1 + 0 = cloud_color"""
    return (one_pixel((8.0, 16.0, 8.0), (0.0, 1.0, 0.0), flags=SK.CLOUDS, cloud_cover=1.0, cloud_sharp=2.0 ** 20), [1.0, 1.0, 1.0],
            (1, 0, 0, 0, 1, 0))


HAND_CASES = [zenith, horizon_with_glow, straight_at_the_sun, ground, lambda: ground(-0.5), hit_before_the_fog, hit_in_the_fog, hit_far_away,
              hit_without_fog, hit_with_axis_field_3, hit_along_the_face, hit_behind_the_camera, nan_on_a_hit, nan_on_a_miss,
              camera_above_the_clouds, cloud_coordinate_out_of_range, no_cloud_cover, full_cloud_cover]


def ortho_frame():
    """an ortho frame looking up at a slant without clouds: every pixel a miss, every ray the same direction: one colour"""
    cam = tuple(np.asarray(v, F32) for v in ((50.0, 20.0, 50.0), (0.25, 0.5, 0.75), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)))
    return dict(color=np.full((8, 8, 3), 0.5, F32), keys=np.zeros((8, 8), np.uint32), cam=cam, ortho=True, ortho_size=(4.0, 4.0), params=dict(HAND))
