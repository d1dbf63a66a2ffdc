"""Two restatements of the frame denoiser (include/vxrt.h, vxrt_frame_guides / vxrt_denoise_frame) from its definition, never
from the code under test: the guide keys and the a-trous filter each as vectorised numpy (25 shifted array operations per
iteration, in the contract's tap order) and as a scalar loop over pixels with np.float32 scalars.  Every operation is a
binary32 operation in the order the header gives.  The primary rays come from the restated camera of
tests/render_edge_cases.py (camera_rays), normalised as the renderer normalises them."""
from types import SimpleNamespace

import numpy as np

from tests.render_edge_cases import camera_rays

F32 = np.float32
H3 = (F32(0.375), F32(0.25), F32(0.0625))
MAX_SIDE, MAX_PIXELS, MAX_ITERATIONS, MAX_AXIS = 65535, 1 << 26, 6, 1 << 24
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def frame_ok(W, H):
    return 1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE and W * H <= MAX_PIXELS


def workspace_bytes(W, H):
    """the formula of include/vxrt.h"""
    return 2 * W * H * 16 if frame_ok(W, H) else 0


def primary_rays(W, H, pos, fwd, up, right, ortho=False, fov=90.0, ortho_size=(10.0, 10.0), rows=None):
    """(origins, directions), each (H, W, 3) binary32: the perspective direction normalised (v * (1 / sqrt(dot(v, v)))), the
    ortho direction fwd as it is; with rows = (y0, y1) the rows y0 .. y1 - 1 of the W x H frame alone"""
    o, d = camera_rays(SimpleNamespace(W=W, H=H, camera=(pos, fwd, up, right), ortho=ortho, ortho_size=ortho_size, fov=fov, rows=rows))
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    if not ortho:
        with np.errstate(**_QUIET):
            dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            d = d * (F32(1) / np.sqrt(dd, dtype=F32))[..., None]
    return o, d


# ---- guide keys ------------------------------------------------------------------------------------------------------
def keys_np(hit, dims, o, d):
    """hit (H, W) int64, dims = (X, Y, Z), o and d (H, W, 3) binary32 -> (H, W) uint32"""
    X, Y, Z = (int(v) for v in dims)
    hit = np.asarray(hit, np.int64)
    ok = (hit >= 0) & (hit < X * Y * Z)
    h = np.where(ok, hit, 0)
    v = np.stack([h % X, (h // X) % Y, h // (X * Y)], -1)
    with np.errstate(**_QUIET):
        p = np.where(d > 0, v, v + 1)
        t = np.where(d != 0, (p.astype(F32) - o) / np.where(d != 0, d, F32(1)), F32(-np.inf)).astype(F32)
    axis = np.zeros(hit.shape, np.int64)
    best = t[..., 0]
    for k in (1, 2):
        better = t[..., k] > best
        axis = np.where(better, k, axis)
        best = np.where(better, t[..., k], best)
    toward = np.take_along_axis(d, axis[..., None], -1)[..., 0] > 0
    plane = np.take_along_axis(p, axis[..., None], -1)[..., 0]
    key = (1 << 31) | (axis << 26) | (toward.astype(np.int64) << 25) | plane
    return np.where(ok, key, 0).astype(np.uint32)


def key_scalar(hit, dims, o, d):
    """one pixel: hit an int, o and d three binary32 each"""
    X, Y, Z = (int(v) for v in dims)
    hit = int(hit)
    if hit < 0 or hit >= X * Y * Z:
        return 0
    v = (hit % X, hit // X % Y, hit // (X * Y))
    t, p = [], []
    for k in range(3):
        dk, ok = F32(d[k]), F32(o[k])
        p.append(v[k] if dk > 0 else v[k] + 1)
        with np.errstate(**_QUIET):
            t.append((F32(p[k]) - ok) / dk if dk != 0 else F32(-np.inf))
    axis = 0
    for k in (1, 2):
        if t[k] > t[axis]:
            axis = k
    return (1 << 31) | (axis << 26) | (int(F32(d[axis]) > 0) << 25) | p[axis]


def keys_scalar(hit, dims, o, d):
    H, W = hit.shape
    return np.array([[key_scalar(hit[y, x], dims, o[y, x], d[y, x]) for x in range(W)] for y in range(H)], np.uint32)


# ---- filter ----------------------------------------------------------------------------------------------------------
def _shifted(a, sx, sy, H, W):
    """a[y + sy, x + sx] where that lies inside the frame (else 0), and the inside mask"""
    out = np.zeros_like(a)
    inside = np.zeros((H, W), bool)
    if abs(sx) < W and abs(sy) < H:
        ys, yd = (slice(sy, H), slice(0, H - sy)) if sy >= 0 else (slice(0, H + sy), slice(-sy, H))
        xs, xd = (slice(sx, W), slice(0, W - sx)) if sx >= 0 else (slice(0, W + sx), slice(-sx, W))
        out[yd, xd] = a[ys, xs]
        inside[yd, xd] = True
    return out, inside


def iterate_np(c, keys, step, k):
    """one iteration: c (H, W, 3) binary32, keys (H, W) uint32"""
    H, W = keys.shape
    k = F32(k)
    sw = np.zeros((H, W), F32)
    sc = np.zeros((H, W, 3), F32)
    with np.errstate(**_QUIET):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, inside = _shifted(c, step * dx, step * dy, H, W)
                kq, _ = _shifted(keys, step * dx, step * dy, H, W)
                use = inside & (kq == keys)
                w = np.full((H, W), H3[abs(dx)] * H3[abs(dy)], F32)
                if k > 0:
                    e = cq - c
                    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                    stop = F32(1) - d2 * k
                    w = w * np.where(stop > 0, stop, F32(0))
                sw = np.where(use, sw + w, sw)
                sc = np.where(use[..., None], sc + w[..., None] * cq, sc)
        out = np.where((keys != 0)[..., None], sc / np.where(keys != 0, sw, F32(1))[..., None], c)
    return out.astype(F32)


def denoise_np(color, keys, iterations, k):
    c = np.ascontiguousarray(color, F32)
    keys = np.ascontiguousarray(keys, np.uint32)
    for i in range(iterations):
        c = iterate_np(c, keys, 1 << i, k)
    return c


def iterate_scalar(c, keys, step, k):
    H, W = keys.shape
    k = F32(k)
    src = [[tuple(F32(v) for v in c[y, x]) for x in range(W)] for y in range(H)]
    ks = keys.tolist()
    out = np.empty((H, W, 3), F32)
    zero, one = F32(0), F32(1)
    with np.errstate(**_QUIET):
        for y in range(H):
            for x in range(W):
                kp, p = ks[y][x], src[y][x]
                if kp == 0:
                    out[y, x] = p
                    continue
                sw = sr = sg = sb = zero
                for dy in range(-2, 3):
                    qy = y + step * dy
                    if qy < 0 or qy >= H:
                        continue
                    for dx in range(-2, 3):
                        qx = x + step * dx
                        if qx < 0 or qx >= W or ks[qy][qx] != kp:
                            continue
                        q = src[qy][qx]
                        w = H3[abs(dx)] * H3[abs(dy)]
                        if k > 0:
                            er, eg, eb = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                            d2 = (er * er + eg * eg) + eb * eb
                            stop = one - d2 * k
                            w = w * (stop if stop > 0 else zero)
                        sw = sw + w
                        sr = sr + w * q[0]
                        sg = sg + w * q[1]
                        sb = sb + w * q[2]
                out[y, x] = (sr / sw, sg / sw, sb / sw)
    return out


def denoise_scalar(color, keys, iterations, k):
    c = np.ascontiguousarray(color, F32)
    keys = np.ascontiguousarray(keys, np.uint32)
    for i in range(iterations):
        c = iterate_scalar(c, keys, 1 << i, k)
    return c


def bgra8(color):
    """setPixelColor's rule: clamp, * 255, truncate; bytes b, g, r, 255 -> (H, W, 4) uint8"""
    c = np.ascontiguousarray(color, F32)
    with np.errstate(**_QUIET):
        c = np.where(c > 0, c, F32(0))
        c = np.where(c < 1, c, F32(1))
        b = (c * F32(255)).astype(np.uint32)
    out = np.empty(c.shape[:2] + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = b[..., 2], b[..., 1], b[..., 0], 255
    return out


def bits(a):
    """binary32 array -> its bits, every NaN as one canonical quiet NaN"""
    a = np.ascontiguousarray(a, F32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


# ---- random frames of the tests (shared by the host and the GPU tests) -------------------------------------------------
FRAMES = [(1, 1), (7, 5), (64, 1), (65, 33), (130, 70)]
ITERATIONS = (1, 2, 3, 4, 5, 6)
SCALES = (0.0, 0.75)


def random_frame(W, H, seed=0):
    """colours including 0, negatives and 1e30; keys drawn from a few values plus misses, in patches and in speckle"""
    rng = np.random.default_rng(1000 * W + H + seed)
    c = rng.random((H, W, 3)).astype(F32)
    pick = rng.random((H, W))
    c[pick < 0.05] = 0
    c[(pick >= 0.05) & (pick < 0.10)] *= F32(-1)
    c[(pick >= 0.10) & (pick < 0.12)] = F32(1e30)
    c[(pick >= 0.12) & (pick < 0.14), 1] = F32(-1e30)
    values = np.array([0, 0x80000005, 0x84000005, 0x8A000007, 0x82000005, 0x89FFFFFF], np.uint32)
    coarse = rng.integers(0, len(values), ((H + 7) // 8, (W + 7) // 8))
    idx = np.kron(coarse, np.ones((8, 8), np.int64))[:H, :W]
    speckle = rng.random((H, W)) < 0.15
    idx = np.where(speckle, rng.integers(0, len(values), (H, W)), idx)
    return c, values[idx]
