"""Two restatements of the temporal filter (include/vxrt.h, vxrt_reproject_frame) from its definition, never from the code
under test: vectorised numpy (the four taps as four gathers, in the contract's order) and a scalar loop over pixels with
np.float32 scalars.  Every operation is a binary32 operation in the order the header gives.  The primary rays are those of
tests/ref_denoise.py (primary_rays), the camera constants those of the restated camera of tests/render_edge_cases.py."""
import numpy as np

from tests import ref_denoise as R

F32 = np.float32
MAX_HISTORY = 65535
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def history_ok(max_history):
    return 1 <= max_history <= MAX_HISTORY


def camera_constants(W, H, fov=90.0, ortho_size=(10.0, 10.0)):
    """(kx, ky, ortho_x, ortho_y, ratio) of a W x H launch: what camera_rays (tests/render_edge_cases.py) computes per call"""
    ratio = F32(W) / F32(H)
    ky = np.tan(F32(float(fov) * 3.1415 / 180.0) / F32(2), dtype=F32)
    return ky * ratio, ky, F32(ortho_size[0]), F32(ortho_size[1]), ratio


def _pose(cam):
    return [np.asarray(v, F32) for v in cam]


# ---- vectorised ------------------------------------------------------------------------------------------------------
def reproject_np(color, keys, o, d, prev, consts, hist=None, keys_prev=None, max_history=32, ortho=False, rows=None, frame_h=None,
                 hist_rows=None):
    """color (H, W, 3) binary32, keys (H, W) uint32, (o, d) the primary rays under the current camera (H, W, 3), prev the
    previous camera (origin, fwd, up, right), consts = camera_constants(...), hist (H, W, 4) and keys_prev (H, W) or None
    -> (records (H, W, 4) binary32, (hit, reused, offscreen, rejected)).
    With rows = (y0, y1): a band of a frame of frame_h rows -- color, keys, o and d hold the rows y0 .. y1 - 1, hist and
    keys_prev the rows hist_rows[0] .. hist_rows[1] - 1 of the previous frame, and every tap inside the frame is asserted to
    lie in them; the counts are the band's"""
    c = np.ascontiguousarray(color, F32)
    k = np.ascontiguousarray(keys, np.uint32)
    Hb, W = k.shape
    H = Hb if rows is None else int(frame_h)
    h0, h1 = (0, H) if rows is None else hist_rows
    assert rows is None or (rows[1] - rows[0] == Hb and 0 <= h0 < h1 <= H)
    kx, ky, ortho_x, ortho_y, ratio = consts
    po, pf, pu, pr = _pose(prev)
    hitm = k != 0
    a = ((k >> np.uint32(26)) & np.uint32(31)).astype(np.int64)
    pl = (k & np.uint32(0x1FFFFFF)).astype(F32)

    def dot(u, v):
        return (u[..., 0] * v[0] + u[..., 1] * v[1]) + u[..., 2] * v[2]

    with np.errstate(**_QUIET):
        oa = np.take_along_axis(o, a[..., None], -1)[..., 0]
        da = np.take_along_axis(d, a[..., None], -1)[..., 0]
        t = (pl - oa) / da
        on = hitm & (da != 0) & np.isfinite(t)
        P = o + t[..., None] * d
        P = np.where(np.arange(3) == a[..., None], pl[..., None], P).astype(F32)
        r = P - po
        if ortho:
            su = dot(r, pr) / (ortho_x * ratio)
            sv = dot(r, pu) / ortho_y
        else:
            z = dot(r, pf)
            on = on & (z > 0)
            su = dot(r, pr) / (z * kx)
            sv = dot(r, pu) / (z * ky)
        fx = ((su + F32(1)) * F32(0.5)) * F32(W)
        fy = ((sv + F32(1)) * F32(0.5)) * F32(H)
        on = on & (fx >= -1) & (fx <= W) & (fy >= -1) & (fy <= H)
        fx, fy = np.where(on, fx, F32(0)), np.where(on, fy, F32(0))
        flx, fly = np.floor(fx), np.floor(fy)
        wx, wy = fx - flx, fy - fly
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        weights = ((F32(1) - wx) * (F32(1) - wy), wx * (F32(1) - wy), (F32(1) - wx) * wy, wx * wy)
        sw = np.zeros((Hb, W), F32)
        sc = np.zeros((Hb, W, 3), F32)
        nmin = np.full((Hb, W), np.inf, F32)
        any_inside = np.zeros((Hb, W), bool)
        any_used = np.zeros((Hb, W), bool)
        for j, w in enumerate(weights):
            qx, qy = x0 + (j & 1), y0 + (j >> 1)
            inside = on & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            any_inside |= inside
            if hist is None or keys_prev is None:
                continue
            assert (~inside | ((qy >= h0) & (qy < h1))).all(), "a tap outside the history rows given"
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy - h0, 0, h1 - h0 - 1)
            hq, kq = hist[cy, cx], keys_prev[cy, cx]
            use = inside & (w > 0) & (kq == k) & (hq[..., 3] >= 1)
            any_used |= use
            sw = np.where(use, sw + w, sw)
            sc = np.where(use[..., None], sc + w[..., None] * hq[..., :3], sc)
            nmin = np.where(use & (hq[..., 3] < nmin), hq[..., 3], nmin)
        m = sc / sw[..., None]
        n1 = nmin + F32(1)
        n = np.where(n1 < F32(max_history), n1, F32(max_history))
        blend = m + (c - m) / n[..., None]
    rec = np.empty((Hb, W, 4), F32)
    rec[..., :3] = np.where(any_used[..., None], blend, c)
    rec[..., 3] = np.where(any_used, n, np.where(hitm, F32(1), F32(0)))
    summary = (int(hitm.sum()), int(any_used.sum()), int((hitm & ~any_inside).sum()), int((hitm & any_inside & ~any_used).sum()))
    return rec, summary


# ---- scalar ----------------------------------------------------------------------------------------------------------
def reproject_scalar(color, keys, o, d, prev, consts, hist=None, keys_prev=None, max_history=32, ortho=False):
    """the same, pixel by pixel and step by step as the header numbers them"""
    H, W = keys.shape
    kx, ky, ortho_x, ortho_y, ratio = (F32(v) for v in consts)
    po, pf, pu, pr = ([F32(x) for x in v] for v in _pose(prev))
    one, half, zero = F32(1), F32(0.5), F32(0)
    rec = np.empty((H, W, 4), F32)
    counts = dict(hit=0, reused=0, offscreen=0, rejected=0)
    have = hist is not None and keys_prev is not None

    def dot(u, v):
        return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    def position(k, ov, dv):
        """(fx, fy) in the previous frame, or None: steps 2 and 3"""
        a = (k >> 26) & 31
        pl = F32(k & 0x1FFFFFF)
        if dv[a] == 0:
            return None
        t = (pl - ov[a]) / dv[a]
        if not np.isfinite(t):
            return None
        P = [pl if j == a else ov[j] + t * dv[j] for j in range(3)]
        r = [P[j] - po[j] for j in range(3)]
        if ortho:
            su = dot(r, pr) / (ortho_x * ratio)
            sv = dot(r, pu) / ortho_y
        else:
            z = dot(r, pf)
            if not z > 0:
                return None
            su = dot(r, pr) / (z * kx)
            sv = dot(r, pu) / (z * ky)
        fx = ((su + one) * half) * F32(W)
        fy = ((sv + one) * half) * F32(H)
        if not (fx >= -1 and fx <= W and fy >= -1 and fy <= H):
            return None
        return fx, fy

    with np.errstate(**_QUIET):
        for y in range(H):
            for x in range(W):
                k = int(keys[y, x])
                c = [F32(v) for v in color[y, x]]
                if k == 0:
                    rec[y, x] = (*c, zero)
                    continue
                counts["hit"] += 1
                rec[y, x] = (*c, one)
                f = position(k, [F32(v) for v in o[y, x]], [F32(v) for v in d[y, x]])
                if f is None:
                    counts["offscreen"] += 1
                    continue
                fx, fy = f
                flx, fly = np.floor(fx), np.floor(fy)
                wx, wy = fx - flx, fy - fly
                x0, y0 = int(flx), int(fly)
                taps = (((x0, y0), (one - wx) * (one - wy)), ((x0 + 1, y0), wx * (one - wy)),
                        ((x0, y0 + 1), (one - wx) * wy), ((x0 + 1, y0 + 1), wx * wy))
                sw = sr = sg = sb = zero
                nmin = F32(np.inf)
                inside = used = 0
                for (qx, qy), w in taps:
                    if qx < 0 or qy < 0 or qx >= W or qy >= H:
                        continue
                    inside += 1
                    if not have or not w > 0 or int(keys_prev[qy, qx]) != k:
                        continue
                    h = [F32(v) for v in hist[qy, qx]]
                    if not h[3] >= 1:
                        continue
                    used += 1
                    sw = sw + w
                    sr, sg, sb = sr + w * h[0], sg + w * h[1], sb + w * h[2]
                    nmin = h[3] if h[3] < nmin else nmin
                if inside == 0:
                    counts["offscreen"] += 1
                elif used == 0:
                    counts["rejected"] += 1
                else:
                    counts["reused"] += 1
                    n1 = nmin + one
                    n = n1 if n1 < F32(max_history) else F32(max_history)
                    m = (sr / sw, sg / sw, sb / sw)
                    rec[y, x] = (*[m[j] + (c[j] - m[j]) / n for j in range(3)], n)
    return rec, (counts["hit"], counts["reused"], counts["offscreen"], counts["rejected"])


def reproject(color, keys, cur, prev, hist=None, keys_prev=None, max_history=32, ortho=False, fov=90.0, ortho_size=(10.0, 10.0),
              scalar=False):
    """the call as the library takes it: the cameras as (origin, fwd, up, right)"""
    H, W = keys.shape
    o, d = R.primary_rays(W, H, *cur, ortho=ortho, fov=fov, ortho_size=ortho_size)
    f = reproject_scalar if scalar else reproject_np
    return f(color, keys, o, d, prev, camera_constants(W, H, fov, ortho_size), hist, keys_prev, max_history, ortho)


# ---- random frames of the tests (shared by the host and the GPU tests) -------------------------------------------------
FRAMES = R.FRAMES + [(64, 4), (65, 5)]
FOREIGN = 0x88000009  # a key of the previous frame that no current pixel has: NaN colours sit behind it
RANDOM_MAX_HISTORY = 7
ORTHO_SIZE = (6.0, 5.0)


def _rot(v, axis, angle):
    """v turned about a coordinate axis (binary64, stored as binary32: the poses need not be orthonormal to the last bit)"""
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    out = np.array(v, np.float64)
    out[i], out[j] = c * v[i] - s * v[j], s * v[i] + c * v[j]
    return out


def random_case(W, H, ortho, seed=0):
    """a frame of R.random_frame's colours and keys, a camera above the planes the keys name looking down at a slant, a
    previous camera a small move away, previous keys that agree with the current ones in most places, and a history with
    n = 0, n = 1 .. RANDOM_MAX_HISTORY and NaN colours behind FOREIGN keys; everything read-only"""
    rng = np.random.default_rng(77 * W + 13 * H + 2 * seed + int(ortho))
    color, keys = R.random_frame(W, H, seed)
    fwd, up, right = np.array([0.3, -0.9, 0.2]), np.array([0.1, 0.2, 0.95]), np.array([0.95, 0.3, -0.1])
    pos = np.array([9.0, 14.0, 6.0])
    cur = tuple(np.asarray(v, F32) for v in (pos, fwd, up, right))
    ang = rng.uniform(-0.03, 0.03, 3)
    turned = [fwd, up, right]
    for axis in range(3):
        turned = [_rot(v, axis, ang[axis]) for v in turned]
    prev = tuple(np.asarray(v, F32) for v in (pos + rng.uniform(-0.4, 0.4, 3), *turned))
    keys_prev = np.roll(keys, (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))), (0, 1)).copy()
    pick = rng.random((H, W))
    keys_prev[pick < 0.10] = FOREIGN
    keys_prev[(pick >= 0.10) & (pick < 0.15)] = 0
    hist = np.empty((H, W, 4), F32)
    hist[..., :3] = rng.integers(0, 1025, (H, W, 3)) / 1024.0
    hist[..., 3] = rng.choice(np.array([0, 1, 1, 2, 3, 5, RANDOM_MAX_HISTORY, RANDOM_MAX_HISTORY], F32), (H, W))
    hist[keys_prev == FOREIGN, :3] = np.nan
    hist[keys_prev == 0, 3] = 0
    for a in (color, keys, keys_prev, hist):
        a.setflags(write=False)
    return dict(color=color, keys=keys, cur=cur, prev=prev, hist=hist, keys_prev=keys_prev, ortho=ortho,
                max_history=RANDOM_MAX_HISTORY, ortho_size=ORTHO_SIZE)


def run_case(case, scalar=False, history=True):
    return reproject(case["color"], case["keys"], case["cur"], case["prev"], case["hist"] if history else None,
                     case["keys_prev"] if history else None, case["max_history"], case["ortho"], ortho_size=case["ortho_size"],
                     scalar=scalar)
