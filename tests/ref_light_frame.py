"""Two restatements of the light on frames (include/vxrt.h, vxrt_light_frame) from its definition, never from the code under
test: vectorised numpy over the whole frame (the nine cells as nine gathers) and a scalar loop over pixels with np.float32
scalars.  Every float operation is a binary32 operation in the order the header gives.  The primary rays and the guide keys
are those of tests/ref_denoise.py (primary_rays, keys_np).  The world is a bool array indexed [x, y, z], the levels a uint8
array indexed [x, y, z] over the light box (what tests/ref_light.py returns), or None."""
import numpy as np

from tests import ref_denoise as R

F32 = np.float32
SMOOTH, OCCLUSION = 1, 2
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")
DEFAULTS = dict(flags=SMOOTH | OCCLUSION, outside_level=0xF0, sky_floor=0.25, block_color=(1.0, 0.8, 0.5), ao_curve=(0.4, 0.6, 0.8, 1.0))


def _params(params):
    p = dict(DEFAULTS)
    p.update(params or {})
    return (int(p["flags"]), int(p["outside_level"]), F32(p["sky_floor"]), [F32(v) for v in p["block_color"]],
            [F32(v) for v in p["ao_curve"]])


def _clamp(x):
    return np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)


# ---- vectorised ------------------------------------------------------------------------------------------------------
def light_frame_np(color, keys, hit, o, d, world, levels, box, params=None, solid=None):
    """color (H, W, 3) binary32, keys (H, W) uint32, hit (H, W) int64, (o, d) the primary rays (H, W, 3), world bool [x, y, z],
    levels uint8 [x, y, z] over box = (origin, dims) or None -> (colour (H, W, 3), terms (H, W, 3), (hit, in_box, occluded,
    dark), info); info: what the frame exercises, for the tests of the case sets.  With `solid` given, `world` is the
    world's extents (X, Y, Z) alone and solid(q), q an integer array (..., 3) of voxels inside the world, says which are
    solid: for worlds too large for a dense array"""
    flags, outside, sky_floor, block_color, ao_curve = _params(params)
    c = np.ascontiguousarray(color, F32)
    k = np.ascontiguousarray(keys, np.uint32)
    hit = np.asarray(hit, np.int64)
    H, W = k.shape
    X, Y, Z = (int(n) for n in world) if solid is not None else world.shape
    dims = np.array([X, Y, Z])
    bo, bd = np.asarray(box[0], np.int64), np.asarray(box[1], np.int64)
    hitm = (k != 0) & (hit >= 0) & (hit < X * Y * Z)
    h = np.where(hitm, hit, 0)
    v = np.stack([h % X, (h // X) % Y, h // (X * Y)], -1)
    a = np.minimum((k >> np.uint32(26)) & np.uint32(31), 2).astype(np.int64)
    toward = ((k >> np.uint32(25)) & np.uint32(1)).astype(bool)
    pl = (k & np.uint32(0x1FFFFFF)).astype(F32)
    b = np.where(a == 0, 1, 0)
    cc = np.where(a == 2, 1, 2)
    eye = np.eye(3, dtype=np.int64)
    f = v + eye[a] * np.where(toward, -1, 1)[..., None]

    def is_solid(q):
        inside = ((q >= 0) & (q < dims)).all(-1)
        qc = np.clip(q, 0, dims - 1)
        return inside & (world[qc[..., 0], qc[..., 1], qc[..., 2]] if solid is None else np.asarray(solid(qc), bool))

    def in_box(q):
        return np.full(q.shape[:-1], False) if levels is None else ((q >= bo) & (q < bo + bd)).all(-1)

    def lev(q, s):
        inb = in_box(q)
        out = np.full(q.shape[:-1], outside, np.int64)
        if levels is not None:
            r = np.clip(q - bo, 0, bd - 1)
            out = np.where(inb, levels[r[..., 0], r[..., 1], r[..., 2]].astype(np.int64), out)
        return np.where(s, 0, out)

    S, L, B = {}, {}, {}
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            q = f + i * eye[b] + j * eye[cc]
            S[i, j] = is_solid(q)
            L[i, j] = lev(q, S[i, j])
            B[i, j] = in_box(q)
    cells_in_box = sum(B[ij].astype(np.int64) for ij in B)
    corner = {}
    opens, cnts = [], []
    occluded = np.zeros((H, W), bool)
    for j in (0, 1):
        for i in (0, 1):
            si, sj = 2 * i - 1, 2 * j - 1
            s1, s2, s3 = S[si, 0], S[0, sj], S[si, sj]
            members = [(np.ones((H, W), bool), L[0, 0]), (~s1, L[si, 0]), (~s2, L[0, sj]), (~(s3 | (s1 & s2)), L[si, sj])]
            cnt = sum(m.astype(np.int64) for m, _ in members)
            sky = sum(np.where(m, l >> 4, 0) for m, l in members)
            blk = sum(np.where(m, l & 15, 0) for m, l in members)
            opn = np.where(s1 & s2, 0, 3 - (s1.astype(np.int64) + s2 + s3))
            occluded |= opn < 3
            if flags & SMOOTH:
                ls, lb = sky.astype(F32) / cnt.astype(F32), blk.astype(F32) / cnt.astype(F32)
            else:
                ls, lb = (L[0, 0] >> 4).astype(F32), (L[0, 0] & 15).astype(F32)
            ao = np.array(ao_curve, F32)[opn] if flags & OCCLUSION else np.ones((H, W), F32)
            corner[i, j] = (ls, lb, ao)
            opens.append(opn)
            cnts.append(cnt)

    def pick(vec, axis):
        return np.take_along_axis(vec, axis[..., None], -1)[..., 0]

    with np.errstate(**_QUIET):
        da = pick(d, a)
        t = (pl - pick(o, a)) / da
        u_raw = (pick(o, b) + t * pick(d, b)) - pick(v, b).astype(F32)
        w_raw = (pick(o, cc) + t * pick(d, cc)) - pick(v, cc).astype(F32)
        u, w = _clamp(u_raw), _clamp(w_raw)
        centre = (da == 0) | ~np.isfinite(t) | ~np.isfinite(u) | ~np.isfinite(w)
        u, w = np.where(centre, F32(0.5), u), np.where(centre, F32(0.5), w)
        q = []
        for n in range(3):
            q00, q10, q01, q11 = corner[0, 0][n], corner[1, 0][n], corner[0, 1][n], corner[1, 1][n]
            q0 = q00 + u * (q10 - q00)
            q1 = q01 + u * (q11 - q01)
            q.append(q0 + w * (q1 - q0))
        Sk, Bk, A = q[0] / F32(15), q[1] / F32(15), q[2]
        ks = sky_floor + (F32(1) - sky_floor) * Sk
        lit = np.stack([(c[..., ch] * ks + block_color[ch] * Bk) * A for ch in range(3)], -1).astype(F32)
    out = np.where(hitm[..., None], lit, c)
    terms = np.where(hitm[..., None], np.stack([Sk, Bk, A], -1), F32(0)).astype(F32)
    front_in_box = B[0, 0]
    dark = (Sk == 0) & (Bk == 0)
    summary = (int(hitm.sum()), int((hitm & front_in_box).sum()), int((hitm & occluded).sum()), int((hitm & dark).sum()))
    info = dict(hit=hitm, open=np.stack(opens, -1), cnt=np.stack(cnts, -1), low=(u_raw < 0) | (w_raw < 0), high=(u_raw > 1) | (w_raw > 1),
                interior=(u_raw > 0) & (u_raw < 1) & (w_raw > 0) & (w_raw < 1), centre=centre, front_in_box=front_in_box,
                cells_in_box=cells_in_box, front_outside_world=((f < 0) | (f >= dims)).any(-1))
    return out, terms, summary, info


# ---- scalar ----------------------------------------------------------------------------------------------------------
def light_frame_scalar(color, keys, hit, o, d, world, levels, box, params=None):
    """the same, pixel by pixel and step by step as the header words it -> (colour, terms, summary)"""
    flags, outside, sky_floor, block_color, ao_curve = _params(params)
    H, W = keys.shape
    X, Y, Z = world.shape
    bo, bd = [int(x) for x in box[0]], [int(x) for x in box[1]]
    out = np.array(color, F32)
    terms = np.zeros((H, W, 3), F32)
    counts = [0, 0, 0, 0]
    zero, one, half, fifteen = F32(0), F32(1), F32(0.5), F32(15)
    wl = world.tolist()
    ll = None if levels is None else levels.tolist()
    kl, hl = keys.tolist(), np.asarray(hit, np.int64).tolist()

    def solid(q):
        return 0 <= q[0] < X and 0 <= q[1] < Y and 0 <= q[2] < Z and wl[q[0]][q[1]][q[2]]

    def boxed(q):
        return ll is not None and all(bo[n] <= q[n] < bo[n] + bd[n] for n in range(3))

    def lev(q):
        if solid(q):
            return 0
        return ll[q[0] - bo[0]][q[1] - bo[1]][q[2] - bo[2]] if boxed(q) else outside

    def clamp(x):
        return zero if x < 0 else one if x > 1 else x

    def lerp(q00, q10, q01, q11, u, w):
        q0 = q00 + u * (q10 - q00)
        q1 = q01 + u * (q11 - q01)
        return q0 + w * (q1 - q0)

    with np.errstate(**_QUIET):
        for y in range(H):
            for x in range(W):
                key, h = kl[y][x], hl[y][x]
                if key == 0 or h < 0 or h >= X * Y * Z:
                    continue
                v = [h % X, h // X % Y, h // (X * Y)]
                a = min((key >> 26) & 31, 2)
                b, c = (1, 2) if a == 0 else (0, 2) if a == 1 else (0, 1)
                f = list(v)
                f[a] += -1 if (key >> 25) & 1 else 1

                def cell(i, j):
                    q = list(f)
                    q[b] += i
                    q[c] += j
                    return q

                ov, dv = [F32(n) for n in o[y, x]], [F32(n) for n in d[y, x]]
                t = (F32(key & 0x1FFFFFF) - ov[a]) / dv[a] if dv[a] != 0 else F32(np.nan)
                u = clamp((ov[b] + t * dv[b]) - F32(v[b]))
                w = clamp((ov[c] + t * dv[c]) - F32(v[c]))
                if dv[a] == 0 or not (np.isfinite(t) and np.isfinite(u) and np.isfinite(w)):
                    u = w = half
                l00 = lev(cell(0, 0))
                ls, lb, ao = {}, {}, {}
                occluded = False
                for i in (0, 1):
                    for j in (0, 1):
                        si, sj = 2 * i - 1, 2 * j - 1
                        s1, s2, s3 = bool(solid(cell(si, 0))), bool(solid(cell(0, sj))), bool(solid(cell(si, sj)))
                        members = [l00]
                        if not s1:
                            members.append(lev(cell(si, 0)))
                        if not s2:
                            members.append(lev(cell(0, sj)))
                        if not (s3 or (s1 and s2)):
                            members.append(lev(cell(si, sj)))
                        opn = 0 if s1 and s2 else 3 - (s1 + s2 + s3)
                        occluded = occluded or opn < 3
                        if flags & SMOOTH:
                            ls[i, j] = F32(sum(m >> 4 for m in members)) / F32(len(members))
                            lb[i, j] = F32(sum(m & 15 for m in members)) / F32(len(members))
                        else:
                            ls[i, j], lb[i, j] = F32(l00 >> 4), F32(l00 & 15)
                        ao[i, j] = ao_curve[opn] if flags & OCCLUSION else one
                S = lerp(ls[0, 0], ls[1, 0], ls[0, 1], ls[1, 1], u, w) / fifteen
                Bk = lerp(lb[0, 0], lb[1, 0], lb[0, 1], lb[1, 1], u, w) / fifteen
                A = lerp(ao[0, 0], ao[1, 0], ao[0, 1], ao[1, 1], u, w)
                ks = sky_floor + (one - sky_floor) * S
                for ch in range(3):
                    out[y, x, ch] = (F32(color[y, x, ch]) * ks + block_color[ch] * Bk) * A
                terms[y, x] = (S, Bk, A)
                counts[0] += 1
                counts[1] += int(boxed(f))
                counts[2] += int(occluded)
                counts[3] += int(S == 0 and Bk == 0)
    return out, terms, tuple(counts)


def light_frame(color, hit, cam, world, levels=None, box=((0, 0, 0), (1, 1, 1)), params=None, ortho=False, fov=90.0,
                ortho_size=(10.0, 10.0), scalar=False, keys=None, solid=None):
    """the call as the library takes it: the camera as (origin, fwd, up, right); the keys are those of the guide restatement
    unless given -> (colour, terms, summary) and, vectorised, info; `solid` (vectorised only): as light_frame_np takes it"""
    H, W = np.asarray(hit).shape
    o, d = R.primary_rays(W, H, *cam, ortho=ortho, fov=fov, ortho_size=ortho_size)
    if keys is None:
        keys = R.keys_np(hit, world if solid is not None else world.shape, o, d)
    if solid is not None:
        assert not scalar
        return light_frame_np(color, keys, hit, o, d, world, levels, box, params, solid)
    fn = light_frame_scalar if scalar else light_frame_np
    return fn(color, keys, hit, o, d, world, levels, box, params)
