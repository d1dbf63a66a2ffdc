"""Two restatements of the voxel materials (include/vxrt.h, vxrt_material_field / vxrt_material_frame) from their definition,
never from the code under test: vectorised numpy (the run above every voxel as a cumulative count down y over the whole
world, the frame by fancy indexing) and scalar loops per voxel and per pixel that walk up the column as the header words it.
Every float operation is a binary32 operation in the order the header gives.  The primary rays, the guide keys and the
clamp of the position on the face are those of tests/ref_denoise.py and tests/ref_light_frame.py; the frame restatement
also holds its position classes against the ones ref_light_frame.py reports for the same pixels.

The world is a bool array indexed [x, y, z]; rules are rows (y_from or None, top, under, deep, under_depth); paint is a uint8
array [x, y, z] over paint_box = (origin, dims) or None; a palette is (tints float32 (256, 3), tiles (256, 3) top, side,
bottom); the atlas a uint8 array [n_tiles, T, T, 4] or None."""
import numpy as np

from tests import ref_light_frame as LF

F32 = np.float32
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")
NO_TILE = 0xFFFF


def _bands(rules):
    return [(-(1 << 31) if r[0] is None else int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4])) for r in rules]


def runs_of(world):
    """run(v) for every voxel of the world: the consecutive solid voxels directly above it, as int64 [x, y, z]"""
    X, Y, Z = world.shape
    run = np.zeros((X, Y, Z), np.int64)
    for y in range(Y - 2, -1, -1):
        run[:, y, :] = np.where(world[:, y + 1, :], run[:, y + 1, :] + 1, 0)
    return run


def _rule_np(bands, y, run):
    """rule(v) for arrays of altitudes and runs"""
    froms = np.array([b[0] for b in bands], np.int64)
    i = np.searchsorted(froms, np.asarray(y, np.int64), side="right") - 1
    table = np.array([b[1:] for b in bands], np.int64)
    top, under, deep, depth = (table[i, k] for k in range(4))
    return np.where(run == 0, top, np.where(run <= depth, under, deep))


def _paint_np(q, paint, paint_box):
    """the paint byte of the voxels q (..., 3): 0 without paint or outside P"""
    if paint is None:
        return np.zeros(q.shape[:-1], np.int64)
    po, pd = np.asarray(paint_box[0], np.int64), np.asarray(paint_box[1], np.int64)
    inside = ((q >= po) & (q < po + pd)).all(-1)
    r = np.clip(q - po, 0, pd - 1)
    return np.where(inside, paint[r[..., 0], r[..., 1], r[..., 2]].astype(np.int64), 0)


# ---- the field ---------------------------------------------------------------------------------------------------------
def material_field_np(world, origin, dims, rules, paint=None, paint_box=None):
    """-> (bytes uint8 [x, y, z] over the box, (solid, painted, top, hist)) with hist a list of 256 counts"""
    bands = _bands(rules)
    wd = np.array(world.shape)
    q = np.stack(np.meshgrid(*[np.arange(o, o + d, dtype=np.int64) for o, d in zip(origin, dims)], indexing="ij"), -1)
    inside = ((q >= 0) & (q < wd)).all(-1)
    qc = np.clip(q, 0, wd - 1)
    solid = inside & world[qc[..., 0], qc[..., 1], qc[..., 2]]
    run = runs_of(world)[qc[..., 0], qc[..., 1], qc[..., 2]]
    p = _paint_np(q, paint, paint_box)
    m = np.where(p != 0, p, _rule_np(bands, q[..., 1], run))
    out = np.where(solid, m, 0).astype(np.uint8)
    hist = np.bincount(out.reshape(-1), minlength=256).tolist()
    return out, (int(solid.sum()), int((solid & (p != 0)).sum()), int((solid & (run == 0)).sum()), hist)


def _material_scalar(wl, shape, bands, pl, paint_box, v):
    """(material(v), painted, run == 0) of voxel v, walking up as the header words it"""
    X, Y, Z = shape
    band = [b for b in bands if b[0] <= v[1]][-1]
    run = 0
    while run <= band[4]:  # never more than under_depth + 1 voxels up
        y = v[1] + run + 1
        if not (0 <= v[0] < X and 0 <= y < Y and 0 <= v[2] < Z and wl[v[0]][y][v[2]]):
            break
        run += 1
    rule = band[1] if run == 0 else band[2] if run <= band[4] else band[3]
    p = 0
    if pl is not None:
        r = [v[k] - paint_box[0][k] for k in range(3)]
        if all(0 <= r[k] < paint_box[1][k] for k in range(3)):
            p = pl[r[0]][r[1]][r[2]]
    return (p if p else rule), bool(p), run == 0


def material_field_scalar(world, origin, dims, rules, paint=None, paint_box=None):
    bands = _bands(rules)
    X, Y, Z = world.shape
    wl = world.tolist()
    pl = None if paint is None else paint.tolist()
    out = np.zeros(dims, np.uint8)
    solid = painted = top = 0
    hist = [0] * 256
    for i in range(dims[0]):
        for j in range(dims[1]):
            for k in range(dims[2]):
                v = (origin[0] + i, origin[1] + j, origin[2] + k)
                m = 0
                if 0 <= v[0] < X and 0 <= v[1] < Y and 0 <= v[2] < Z and wl[v[0]][v[1]][v[2]]:
                    m, p, t = _material_scalar(wl, world.shape, bands, pl, paint_box, v)
                    solid, painted, top = solid + 1, painted + int(p), top + int(t)
                out[i, j, k] = m
                hist[m] += 1
    return out, (solid, painted, top, hist)


# ---- the frame ---------------------------------------------------------------------------------------------------------
def material_frame_np(color, keys, hit, o, d, world, rules, palette, atlas=None, paint=None, paint_box=None, n_tiles=None):
    """color (H, W, 3) binary32, keys (H, W) uint32, hit (H, W) int64, (o, d) the primary rays -> (colour (H, W, 3), material
    ids uint8 (H, W), (hit, painted, top, textured), info); n_tiles: what the call is told (default: the atlas's tiles)"""
    bands = _bands(rules)
    tints, tiles = np.asarray(palette[0], F32), np.asarray(palette[1], np.int64)
    c = np.ascontiguousarray(color, F32)
    k = np.ascontiguousarray(keys, np.uint32)
    hit = np.asarray(hit, np.int64)
    X, Y, Z = world.shape
    hitm = (k != 0) & (hit >= 0) & (hit < X * Y * Z)
    h = np.where(hitm, hit, 0)
    v = np.stack([h % X, (h // X) % Y, h // (X * Y)], -1)
    a = np.minimum((k >> np.uint32(26)) & np.uint32(31), 2).astype(np.int64)
    toward = ((k >> np.uint32(25)) & np.uint32(1)).astype(bool)
    pl = (k & np.uint32(0x1FFFFFF)).astype(F32)
    b = np.where(a == 0, 1, 0)
    cc = np.where(a == 2, 1, 2)
    run = runs_of(world)[v[..., 0], v[..., 1], v[..., 2]]
    p = _paint_np(v, paint, paint_box)
    m = np.where(p != 0, p, _rule_np(bands, v[..., 1], run))
    cls = np.where(a != 1, 1, np.where(toward, 2, 0))  # top, side, bottom
    tile = tiles[m, cls]

    def pick(vec, axis):
        return np.take_along_axis(vec, axis[..., None], -1)[..., 0]

    T = 1 if atlas is None else atlas.shape[1]
    nt = (0 if atlas is None else atlas.shape[0]) if n_tiles is None else n_tiles
    with np.errstate(**_QUIET):
        da = pick(d, a)
        t = (pl - pick(o, a)) / da
        u_raw = (pick(o, b) + t * pick(d, b)) - pick(v, b).astype(F32)
        w_raw = (pick(o, cc) + t * pick(d, cc)) - pick(v, cc).astype(F32)
        u, w = LF._clamp(u_raw), LF._clamp(w_raw)
        centre = (da == 0) | ~np.isfinite(t) | ~np.isfinite(u) | ~np.isfinite(w)
        u, w = np.where(centre, F32(0.5), u), np.where(centre, F32(0.5), w)
        iu = np.minimum((u * F32(T)).astype(np.int64), T - 1)
        iw = np.minimum((w * F32(T)).astype(np.int64), T - 1)
    s = np.where(a == 0, iw, iu)
    r = np.where(a == 0, T - 1 - iu, np.where(a == 1, iw, T - 1 - iw))
    textured = hitm & (atlas is not None) & (tile < nt)
    tex = np.ones((*k.shape, 3), F32)
    if atlas is not None and atlas.shape[0] > 0:
        texel = atlas[np.clip(tile, 0, atlas.shape[0] - 1), r, s, :3].astype(F32) / F32(255)
        tex = np.where(textured[..., None], texel, tex).astype(F32)
    alb = (tints[m] * tex).astype(F32)
    out = np.where(hitm[..., None], (c * alb).astype(F32), c)
    aov = np.where(hitm, m, 0).astype(np.uint8)
    summary = (int(hitm.sum()), int((hitm & (p != 0)).sum()), int((hitm & (run == 0)).sum()), int(textured.sum()))
    in_p = np.zeros(k.shape, bool) if paint is None else ((v >= np.asarray(paint_box[0])) & (v < np.asarray(paint_box[0]) + np.asarray(paint_box[1]))).all(-1)
    info = dict(hit=hitm, a=a, toward=toward, cls=cls, m=m, run=run, painted=p != 0, in_paint_box=in_p, textured=textured, centre=centre, iu=iu, iw=iw,
                clamped_high=(u_raw > 1) | (w_raw > 1), low=(u_raw < 0) | (w_raw < 0), tile=tile)
    return out, aov, summary, info


def material_frame_scalar(color, keys, hit, o, d, world, rules, palette, atlas=None, paint=None, paint_box=None, n_tiles=None):
    """the same, pixel by pixel -> (colour, material ids, summary)"""
    bands = _bands(rules)
    tints, tiles = np.asarray(palette[0], F32), np.asarray(palette[1], np.int64).tolist()
    H, W = keys.shape
    X, Y, Z = world.shape
    out = np.array(color, F32)
    aov = np.zeros((H, W), np.uint8)
    counts = [0, 0, 0, 0]
    wl = world.tolist()
    pl = None if paint is None else paint.tolist()
    kl, hl = keys.tolist(), np.asarray(hit, np.int64).tolist()
    T = 1 if atlas is None else atlas.shape[1]
    nt = (0 if atlas is None else atlas.shape[0]) if n_tiles is None else n_tiles
    zero, one, half = F32(0), F32(1), F32(0.5)

    def clamp(x):
        return zero if x < 0 else one if x > 1 else x

    with np.errstate(**_QUIET):
        for y in range(H):
            for x in range(W):
                key, h = kl[y][x], hl[y][x]
                if key == 0 or h < 0 or h >= X * Y * Z:
                    continue
                v = [h % X, h // X % Y, h // (X * Y)]
                a = min((key >> 26) & 31, 2)
                toward = (key >> 25) & 1
                b, c = (1, 2) if a == 0 else (0, 2) if a == 1 else (0, 1)
                m, painted, top = _material_scalar(wl, world.shape, bands, pl, paint_box, v)
                ov, dv = [F32(n) for n in o[y, x]], [F32(n) for n in d[y, x]]
                t = (F32(key & 0x1FFFFFF) - ov[a]) / dv[a] if dv[a] != 0 else F32(np.nan)
                u = clamp((ov[b] + t * dv[b]) - F32(v[b]))
                w = clamp((ov[c] + t * dv[c]) - F32(v[c]))
                if dv[a] == 0 or not (np.isfinite(t) and np.isfinite(u) and np.isfinite(w)):
                    u = w = half
                tile = tiles[m][1 if a != 1 else 2 if toward else 0]
                tex = [one, one, one]
                if atlas is not None and tile < nt:
                    iu, iw = min(int(u * F32(T)), T - 1), min(int(w * F32(T)), T - 1)
                    if a == 1:
                        s, r = iu, iw
                    elif a == 0:
                        s, r = iw, T - 1 - iu
                    else:
                        s, r = iu, T - 1 - iw
                    tex = [F32(int(atlas[tile, r, s, ch])) / F32(255) for ch in range(3)]
                    counts[3] += 1
                for ch in range(3):
                    alb = tints[m][ch] * tex[ch]
                    out[y, x, ch] = F32(color[y, x, ch]) * alb
                aov[y, x] = m
                counts[0] += 1
                counts[1] += int(painted)
                counts[2] += int(top)
    return out, aov, tuple(counts)
