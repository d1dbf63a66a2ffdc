"""Two restatements of the sky on frames (include/vxrt.h, vxrt_sky_frame) from its definition, never from the code under
test: vectorised numpy over all pixels at once, and a scalar loop over pixels with np.float32 scalars and Python integers.
Every operation is a binary32 operation in the order the header gives.  The primary rays come from
tests/ref_denoise.primary_rays.  Both take a whole frame or a list of pixels of a frame."""
from types import SimpleNamespace

import numpy as np

from tests import ref_denoise as R

F32 = np.float32
U32 = np.uint32
CLOUDS = 1
LIM = F32(2.0 ** 30)
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")
COUNTERS = ("miss", "hit", "ground", "sun", "cloud", "fogged")
# why a hit pixel was copied, and why a miss pixel of the upper half under VXRT_SKY_CLOUDS has no cloud
COPIED = ("d0", "t_not_finite", "t_negative", "no_fog")
NO_CLOUD = ("level", "above", "t_not_finite", "too_far", "range")

# a daytime sky: the default of voxelengine_amd.Sky and of the example's preset
DAY = dict(flags=0, glow_log2=3, octaves=4, seed=1, zenith=(0.18, 0.38, 0.80), horizon=(0.70, 0.82, 0.95), ground=(0.30, 0.28, 0.25),
           sun_color=(1.0, 0.95, 0.80), cloud_color=(1.0, 1.0, 1.0), sun_dir=(0.577, 0.577, 0.577), glow_strength=0.35, ground_fade=4.0,
           cos_inner=0.9995, cos_outer=0.9985, cloud_y=400.0, cloud_scale=0.004, cloud_offset=(0.0, 0.0), cloud_max_t=20000.0,
           cloud_cover=0.5, cloud_sharp=3.0, cloud_fade=6.0, fog_start=64.0, fog_density=0.0015, fog_max=0.85)
VEC3 = ("zenith", "horizon", "ground", "sun_color", "cloud_color", "sun_dir")
SCALARS = ("glow_strength", "ground_fade", "cos_inner", "cos_outer", "cloud_y", "cloud_scale", "cloud_max_t", "cloud_cover", "cloud_sharp",
           "cloud_fade", "fog_start", "fog_density", "fog_max")


def params(p=None):
    """DAY overridden by `p`, as binary32 values, with the normalised sun `sun`"""
    d = dict(DAY, **(p or {}))
    q = SimpleNamespace(flags=int(d["flags"]), glow_log2=int(d["glow_log2"]), octaves=int(d["octaves"]), seed=int(d["seed"]) & 0xFFFFFFFF)
    for k in VEC3:
        setattr(q, k, np.asarray(d[k], F32))
    for k in SCALARS:
        setattr(q, k, F32(d[k]))
    q.cloud_offset = np.asarray(d["cloud_offset"], F32)
    v = q.sun_dir
    with np.errstate(**_QUIET):
        n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], dtype=F32)
        q.sun = (v / n).astype(F32)
    return q


def pixel_rays(W, H, cam, pixels, ortho=False, fov=90.0, ortho_size=(10.0, 10.0)):
    """(origins, directions), each (N, 3), of the pixels (N, 2) holding (x, y) of the W x H frame: primary_rays row by row"""
    pixels = np.asarray(pixels, np.int64).reshape(-1, 2)
    o = np.empty((len(pixels), 3), F32)
    d = np.empty((len(pixels), 3), F32)
    for y in np.unique(pixels[:, 1]):
        ro, rd = R.primary_rays(W, H, *cam, ortho=ortho, fov=fov, ortho_size=ortho_size, rows=(int(y), int(y) + 1))
        sel = pixels[:, 1] == y
        o[sel], d[sel] = ro[0][pixels[sel, 0]], rd[0][pixels[sel, 0]]
    return o, d


# ---- vectorised ------------------------------------------------------------------------------------------------------
def _clamp01(x):
    return np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)


def _mix(a, b, w):
    return a + (b - a) * w


def _smooth(x):
    return (x * x) * (F32(3) - F32(2) * x)


def _value_np(i, j, k):
    m = (i * U32(0x8DA6B343)) ^ (j * U32(0xD8163841)) ^ U32((k * 0xCB1AB31F) & 0xFFFFFFFF)
    m = m ^ (m >> U32(16))
    m = m * U32(0x7FEB352D)
    m = m ^ (m >> U32(15))
    m = m * U32(0x846CA68B)
    m = m ^ (m >> U32(16))
    return (m >> U32(8)).astype(F32) * F32(2.0 ** -24)


def _vnoise_np(qx, qz, k):
    fx, fz = np.floor(qx), np.floor(qz)
    ix, iz = (fx.astype(np.int64) & 0xFFFFFFFF).astype(U32), (fz.astype(np.int64) & 0xFFFFFFFF).astype(U32)
    wx, wz = _smooth(qx - fx), _smooth(qz - fz)
    one = U32(1)
    x0 = _mix(_value_np(ix, iz, k), _value_np(ix + one, iz, k), wx)
    x1 = _mix(_value_np(ix, iz + one, k), _value_np(ix + one, iz + one, k), wx)
    return _mix(x0, x1, wz)


def _base_np(P, h, sd):
    a = F32(1) - h
    a2 = a * a
    a4 = a2 * a2
    g = np.where(sd > 0, sd, F32(0)).astype(F32)
    for _ in range(P.glow_log2):
        g = g * g
    k = P.glow_strength * g
    upper = _mix(P.zenith, P.horizon, a4[:, None]) + P.sun_color * k[:, None]
    lower = _mix(P.horizon, P.ground, _clamp01((-h) * P.ground_fade)[:, None])
    return np.where((h >= 0)[:, None], upper, lower).astype(F32)


def _sky_np(P, o, d, color, keys):
    n = len(keys)
    with np.errstate(**_QUIET):
        h = d[:, 1]
        sd = (d[:, 0] * P.sun[0] + d[:, 1] * P.sun[1]) + d[:, 2] * P.sun[2]
        base = _base_np(P, h, sd)
        miss = keys == 0
        upper = h >= 0
        # the disc
        e = _smooth(_clamp01((sd - P.cos_outer) / (P.cos_inner - P.cos_outer)))
        sky = _mix(base, P.sun_color, e[:, None])
        # the clouds
        want = miss & upper & bool(P.flags & CLOUDS)
        t = (P.cloud_y - o[:, 1]) / h
        px = (o[:, 0] + t * d[:, 0]) * P.cloud_scale + P.cloud_offset[0]
        pz = (o[:, 2] + t * d[:, 2]) * P.cloud_scale + P.cloud_offset[1]
        top = F32(2.0 ** (P.octaves - 1))
        qx, qz = px * top, pz * top
        why = {"level": want & ~(h > 0)}
        left = want & (h > 0)
        why["above"] = left & ~(o[:, 1] < P.cloud_y)
        left = left & (o[:, 1] < P.cloud_y)
        why["t_not_finite"] = left & ~np.isfinite(t)
        left = left & np.isfinite(t)
        why["too_far"] = left & ~(t <= P.cloud_max_t)
        left = left & (t <= P.cloud_max_t)
        inside = (qx > -LIM) & (qx < LIM) & (qz > -LIM) & (qz < LIM)
        why["range"] = left & ~inside
        cloudy = left & inside
        px, pz = np.where(cloudy, px, F32(0)).astype(F32), np.where(cloudy, pz, F32(0)).astype(F32)
        noise = np.zeros(n, F32)
        for i in range(P.octaves):
            noise = noise + F32(2.0 ** -(i + 1)) * _vnoise_np(px * F32(2.0 ** i), pz * F32(2.0 ** i), (P.seed + i) & 0xFFFFFFFF)
        dens = _clamp01((noise - (F32(1) - P.cloud_cover)) * P.cloud_sharp)
        alpha = np.where(cloudy, dens * _clamp01(h * P.cloud_fade), F32(0)).astype(F32)
        clouded = _mix(sky, P.cloud_color, alpha[:, None])
        sky = np.where(cloudy[:, None], clouded, sky)
        sky = np.where(upper[:, None], sky, base)
        # the fog of the hits
        axis = np.minimum((keys >> U32(26)) & U32(31), U32(2)).astype(np.int64)
        pl = (keys & U32(0x1FFFFFF)).astype(F32)
        oa = np.take_along_axis(o, axis[:, None], 1)[:, 0]
        da = np.take_along_axis(d, axis[:, None], 1)[:, 0]
        th = (pl - oa) / da
        hit = ~miss
        copied = {"d0": hit & (da == 0)}
        left = hit & (da != 0)
        copied["t_not_finite"] = left & ~np.isfinite(th)
        left = left & np.isfinite(th)
        copied["t_negative"] = left & ~(th >= 0)
        left = left & (th >= 0)
        u = th - P.fog_start
        u = np.where(u > 0, u, F32(0)).astype(F32)
        x = u * P.fog_density
        f = x / (F32(1) + x)
        f = np.where(f < P.fog_max, f, P.fog_max).astype(F32)
        fogged = left & (f > 0)
        copied["no_fog"] = left & ~(f > 0)
        faded = _mix(color, base, f[:, None])
        out = np.where(miss[:, None], sky, np.where(fogged[:, None], faded, color)).astype(F32)
    flags = dict(miss=miss, hit=hit, ground=miss & (h < 0), sun=miss & upper & (e > 0), cloud=cloudy & (alpha > 0), fogged=fogged)
    return out, flags, dict(copied=copied, no_cloud=why, f=np.where(fogged, f, F32(0)), alpha=alpha)


# ---- scalar ----------------------------------------------------------------------------------------------------------
def _c01(x):
    return F32(0) if x < 0 else F32(1) if x > 1 else x


def _value_s(i, j, k):
    M = 0xFFFFFFFF
    m = ((i * 0x8DA6B343) & M) ^ ((j * 0xD8163841) & M) ^ ((k * 0xCB1AB31F) & M)
    m ^= m >> 16
    m = (m * 0x7FEB352D) & M
    m ^= m >> 15
    m = (m * 0x846CA68B) & M
    m ^= m >> 16
    return F32(m >> 8) * F32(2.0 ** -24)


def _vnoise_s(qx, qz, k):
    fx, fz = np.floor(qx), np.floor(qz)
    ix, iz = int(fx) & 0xFFFFFFFF, int(fz) & 0xFFFFFFFF
    wx, wz = _smooth(qx - fx), _smooth(qz - fz)
    x0 = _mix(_value_s(ix, iz, k), _value_s(ix + 1, iz, k), wx)
    x1 = _mix(_value_s(ix, iz + 1, k), _value_s(ix + 1, iz + 1, k), wx)
    return _mix(x0, x1, wz)


def _base_s(P, h, sd):
    if h >= 0:
        a = F32(1) - h
        a2 = a * a
        a4 = a2 * a2
        g = sd if sd > 0 else F32(0)
        for _ in range(P.glow_log2):
            g = g * g
        k = P.glow_strength * g
        return [_mix(P.zenith[ch], P.horizon[ch], a4) + P.sun_color[ch] * k for ch in range(3)]
    w = _c01((-h) * P.ground_fade)
    return [_mix(P.horizon[ch], P.ground[ch], w) for ch in range(3)]


def _pixel_s(P, o, d, c_in, key):
    """-> (colour, the set of counters the pixel adds to, why it was copied or None, why it has no cloud or None, f, alpha)"""
    h = d[1]
    sd = (d[0] * P.sun[0] + d[1] * P.sun[1]) + d[2] * P.sun[2]
    c = _base_s(P, h, sd)
    zero = F32(0)
    if key == 0:
        counts, why, alpha = {"miss"}, None, zero
        if h < 0:
            counts.add("ground")
        if h >= 0:
            e = _smooth(_c01((sd - P.cos_outer) / (P.cos_inner - P.cos_outer)))
            if e > 0:
                counts.add("sun")
            c = [_mix(c[ch], P.sun_color[ch], e) for ch in range(3)]
            if P.flags & CLOUDS:
                t = (P.cloud_y - o[1]) / h if h > 0 and o[1] < P.cloud_y else zero
                if not h > 0:
                    why = "level"
                elif not o[1] < P.cloud_y:
                    why = "above"
                elif not np.isfinite(t):
                    why = "t_not_finite"
                elif not t <= P.cloud_max_t:
                    why = "too_far"
                else:
                    px = (o[0] + t * d[0]) * P.cloud_scale + P.cloud_offset[0]
                    pz = (o[2] + t * d[2]) * P.cloud_scale + P.cloud_offset[1]
                    top = F32(2.0 ** (P.octaves - 1))
                    qx, qz = px * top, pz * top
                    if not (qx > -LIM and qx < LIM and qz > -LIM and qz < LIM):
                        why = "range"
                    else:
                        n = zero
                        for i in range(P.octaves):
                            n = n + F32(2.0 ** -(i + 1)) * _vnoise_s(px * F32(2.0 ** i), pz * F32(2.0 ** i), (P.seed + i) & 0xFFFFFFFF)
                        dens = _c01((n - (F32(1) - P.cloud_cover)) * P.cloud_sharp)
                        alpha = dens * _c01(h * P.cloud_fade)
                        if alpha > 0:
                            counts.add("cloud")
                        c = [_mix(c[ch], P.cloud_color[ch], alpha) for ch in range(3)]
        return c, counts, None, why, zero, alpha
    a = min((key >> 26) & 31, 2)
    pl = F32(key & 0x1FFFFFF)
    t = (pl - o[a]) / d[a]
    if d[a] == 0:
        return list(c_in), {"hit"}, "d0", None, zero, zero
    if not np.isfinite(t):
        return list(c_in), {"hit"}, "t_not_finite", None, zero, zero
    if t < 0:
        return list(c_in), {"hit"}, "t_negative", None, zero, zero
    u = t - P.fog_start
    u = u if u > 0 else zero
    x = u * P.fog_density
    f = x / (F32(1) + x)
    f = f if f < P.fog_max else P.fog_max
    if not f > 0:
        return list(c_in), {"hit"}, "no_fog", None, zero, zero
    return [_mix(c_in[ch], c[ch], f) for ch in range(3)], {"hit", "fogged"}, None, None, f, zero


def _sky_scalar(P, o, d, color, keys):
    n = len(keys)
    out = np.empty((n, 3), F32)
    flags = {k: np.zeros(n, bool) for k in COUNTERS}
    copied = {k: np.zeros(n, bool) for k in COPIED}
    no_cloud = {k: np.zeros(n, bool) for k in NO_CLOUD}
    fs, alphas = np.zeros(n, F32), np.zeros(n, F32)
    with np.errstate(**_QUIET):
        for i in range(n):
            c, counts, why, cloudless, f, alpha = _pixel_s(P, [F32(v) for v in o[i]], [F32(v) for v in d[i]], [F32(v) for v in color[i]],
                                                           int(keys[i]))
            out[i] = c
            for k in counts:
                flags[k][i] = True
            if why:
                copied[why][i] = True
            if cloudless:
                no_cloud[cloudless][i] = True
            fs[i], alphas[i] = f, alpha
    return out, flags, dict(copied=copied, no_cloud=no_cloud, f=fs, alpha=alphas)


# ---- the call --------------------------------------------------------------------------------------------------------
def sky_frame(color, keys, cam, p=None, ortho=False, fov=90.0, ortho_size=(10.0, 10.0), scalar=False, pixels=None, dims=None):
    """vxrt_sky_frame restated.  A whole frame: color (H, W, 3) binary32 and keys (H, W) uint32.  A list of pixels: `pixels`
    (N, 2) holding (x, y) of a frame of `dims` = (W, H), color (N, 3) and keys (N,).  cam = (origin, fwd, up, right); p
    overrides DAY.  -> (colours shaped as `color`, the summary (miss, hit, ground, sun, cloud, fogged) over the pixels given,
    info: the per-pixel flags of every counter, `copied` and `no_cloud` by reason, f and alpha)"""
    P = params(p)
    color = np.ascontiguousarray(color, F32)
    keys = np.ascontiguousarray(keys).view(U32) if np.asarray(keys).dtype.itemsize == 4 else np.asarray(keys, U32)
    shape = color.shape
    if pixels is None:
        H, W = keys.shape
        o, d = R.primary_rays(W, H, *cam, ortho=ortho, fov=fov, ortho_size=ortho_size)
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    else:
        W, H = dims
        o, d = pixel_rays(W, H, cam, pixels, ortho, fov, ortho_size)
    out, flags, info = (_sky_scalar if scalar else _sky_np)(P, o, d, color.reshape(-1, 3), keys.reshape(-1))
    summary = tuple(int(flags[k].sum()) for k in COUNTERS)
    info = dict(info, **flags)
    return out.reshape(shape), summary, info
