"""Restatements of mesh voxelization (include/vxrt.h, vxrt_voxelize_mesh) in numpy and exact rationals, the mesh generators of
its tests and the region packing.  Two forms per field, independent of each other and of the kernels' code:

surface   surface_sat: the 13-axis separating-axis test in int64, the vertices taken relative to each cube's doubled centre;
          surface_clip: the triangle clipped against the cube's six half-spaces in exact rationals (fractions), set when
          something is left -- a point or a segment included.
solid     solid_sign: per voxel, the top-left coverage of (cy, cz) and the sign of the plane at the centre;
          solid_threshold: per (triangle, column) m = ceil((x* - 128) / 256) by one floor division, one toggle at m - 1 and a
          suffix XOR along x.

voxelize() is the fast pair (surface_sat, solid_threshold) with the summary; the tests assert the slow forms equal to it on
every case small enough for them."""
from fractions import Fraction

import numpy as np

SURFACE, SOLID = 1, 2
UNIT, MAX_COORD, MAX_DIM = 256, 1 << 18, 1024


# ---- triangles ------------------------------------------------------------------------------------------------------------
def triangles(verts, tris, dims):
    """the coordinates (m, 3, 3) int64 of the valid, non-degenerate triangles, and (triangles, invalid, degenerate, outside)"""
    v = np.asarray(verts, np.int64).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    if not len(t):
        return np.zeros((0, 3, 3), np.int64), (0, 0, 0, 0)
    ok = (t < len(v)).all(1)
    P = np.zeros((len(t), 3, 3), np.int64)
    P[ok] = v[t[ok]]
    ok &= (np.abs(P) <= MAX_COORD).all((1, 2))
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    deg = ok & (n == 0).all(1)
    outside = ok & ((P.max(1) < 0) | (P.min(1) > UNIT * np.asarray(dims, np.int64))).any(1)
    return P[ok & ~deg], (len(t), int((~ok).sum()), int(deg.sum()), int(outside.sum()))


def _normal(p):
    e, g = p[1] - p[0], p[2] - p[0]
    return np.array([e[1] * g[2] - e[2] * g[1], e[2] * g[0] - e[0] * g[2], e[0] * g[1] - e[1] * g[0]], np.int64)


def _voxel_box(p, dims):
    """the voxels whose closed cube meets the closed bounding box, cut to the region (inclusive)"""
    lo = np.maximum((p.min(0) - 1) >> 8, 0)
    hi = np.minimum(p.max(0) >> 8, np.asarray(dims) - 1)
    return lo, hi


# ---- surface ----------------------------------------------------------------------------------------------------------------
def _surface_tri(g, p):
    lo, hi = _voxel_box(p, g.shape)
    if (lo > hi).any():
        return
    u, n = 2 * p, _normal(p)  # doubled: cube i has the centre 512 i + 256 and the half size 256
    c = [512 * np.arange(lo[k], hi[k] + 1, dtype=np.int64) + 256 for k in range(3)]
    keep2 = []
    for e in range(3):
        f = p[(e + 1) % 3] - p[e]
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            a1, a2 = -f[k2], f[k1]
            pr = a1 * (u[:, k1][:, None, None] - c[k1][None, :, None]) + a2 * (u[:, k2][:, None, None] - c[k2][None, None, :])
            r = 256 * (abs(a1) + abs(a2))
            m = ~((pr.min(0) > r) | (pr.max(0) < -r))  # indexed (k1, k2)
            keep2.append(m[None, :, :] if k == 0 else (m.T[:, None, :] if k == 1 else m[:, :, None]))
    rn = 256 * int(np.abs(n).sum())
    nxy = (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1)
    step = max(1, (1 << 22) // int(nxy))
    for z0 in range(0, len(c[2]), step):
        z1 = min(z0 + step, len(c[2]))
        val = (n[0] * (u[0, 0] - c[0]))[:, None, None] + (n[1] * (u[0, 1] - c[1]))[None, :, None] + \
            (n[2] * (u[0, 2] - c[2][z0:z1]))[None, None, :]
        keep = np.abs(val) <= rn
        for i, m in enumerate(keep2):  # the masks of axis z have no extent along z
            keep &= m if i % 3 == 2 else m[:, :, z0:z1]
        g[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2] + z0:lo[2] + z1] |= keep


def surface_sat(verts, tris, dims):
    g = np.zeros(tuple(dims), bool)
    for p in triangles(verts, tris, dims)[0]:
        _surface_tri(g, p)
    return g


def _clip(poly, k, bound, sign):
    """the part of the closed polygon with sign * (x_k - bound) >= 0, exact"""
    out = []
    for i, a in enumerate(poly):
        b = poly[(i + 1) % len(poly)]
        da, db = sign * (a[k] - bound), sign * (b[k] - bound)
        if da >= 0:
            out.append(a)
        if (da > 0 and db < 0) or (da < 0 and db > 0):
            t = Fraction(da) / Fraction(da - db)
            out.append(tuple(a[j] + t * (b[j] - a[j]) for j in range(3)))
    return out


def triangle_meets_cube(p, voxel):
    poly = [tuple(Fraction(int(x)) for x in q) for q in p]
    for k in range(3):
        for bound, sign in ((UNIT * int(voxel[k]), 1), (UNIT * (int(voxel[k]) + 1), -1)):
            poly = _clip(poly, k, bound, sign)
            if not poly:
                return False
    return True


def surface_clip(verts, tris, dims):
    """slow: every voxel within one voxel of the triangle's bounding box is clipped"""
    g = np.zeros(tuple(dims), bool)
    for p in triangles(verts, tris, dims)[0]:
        lo, hi = _voxel_box(p, dims)
        lo, hi = np.maximum(lo - 1, 0), np.minimum(hi + 1, np.asarray(dims) - 1)
        for x in range(lo[0], hi[0] + 1):
            for y in range(lo[1], hi[1] + 1):
                for z in range(lo[2], hi[2] + 1):
                    if not g[x, y, z] and triangle_meets_cube(p, (x, y, z)):
                        g[x, y, z] = True
    return g


# ---- solid ------------------------------------------------------------------------------------------------------------------
def _cover(q, cy, cz):
    """the top-left coverage of the centres (cy x cz) by the triangle q, oriented with n.x > 0"""
    cov = np.ones((len(cy), len(cz)), bool)
    for e in range(3):
        a, b = q[e], q[(e + 1) % 3]
        ey, ez = -(b[2] - a[2]), b[1] - a[1]
        E = ey * (cy[:, None] - a[1]) + ez * (cz[None, :] - a[2])
        cov &= (E > 0) | ((E == 0) & bool(ey > 0 or (ey == 0 and ez > 0)))
    return cov


def solid_sign(verts, tris, dims):
    g = np.zeros(tuple(dims), bool)
    cx, cy, cz = (UNIT * np.arange(d, dtype=np.int64) + 128 for d in dims)
    for p in triangles(verts, tris, dims)[0]:
        n = _normal(p)
        if n[0] == 0:
            continue
        s = 1 if n[0] > 0 else -1
        cov = _cover(p if s > 0 else p[[0, 2, 1]], cy, cz)
        js, ks = np.nonzero(cov)
        if not len(js):
            continue
        plane = n[0] * (cx[:, None] - p[0, 0]) + (n[1] * (cy[js] - p[0, 1]) + n[2] * (cz[ks] - p[0, 2]))[None, :]
        g[:, js, ks] ^= s * plane < 0
    return g


def solid_threshold(verts, tris, dims):
    tog = np.zeros(tuple(dims), np.uint8)
    for p in triangles(verts, tris, dims)[0]:
        n = _normal(p)
        if n[0] == 0:
            continue
        if n[0] < 0:
            n, q = -n, p[[0, 2, 1]]
        else:
            q = p
        mn, mx = p.min(0), p.max(0)
        jl, jh = max((mn[1] + 127) >> 8, 0), min((mx[1] - 128) >> 8, dims[1] - 1)
        kl, kh = max((mn[2] + 127) >> 8, 0), min((mx[2] - 128) >> 8, dims[2] - 1)
        if jl > jh or kl > kh:
            continue
        cy = UNIT * np.arange(jl, jh + 1, dtype=np.int64) + 128
        cz = UNIT * np.arange(kl, kh + 1, dtype=np.int64) + 128
        cov = _cover(q, cy, cz)
        a = n[0] * (p[0, 0] - 128) - n[1] * (cy[:, None] - p[0, 1]) - n[2] * (cz[None, :] - p[0, 2])
        m = np.clip(-((-a) // (UNIT * n[0])), 0, dims[0])  # ceil by floor division
        js, ks = np.nonzero(cov & (m > 0))
        if len(js):
            np.bitwise_xor.at(tog, (m[js, ks] - 1, js + jl, ks + kl), 1)
    return (np.cumsum(tog[::-1], axis=0, dtype=np.uint8)[::-1] & 1).astype(bool)


# ---- the call ---------------------------------------------------------------------------------------------------------------
def voxelize(verts, tris, dims, modes):
    """{'grid': bool [x, y, z], 'summary': (set, surface, solid, triangles, invalid, degenerate, outside)}"""
    dims = tuple(int(d) for d in dims)
    counts = triangles(verts, tris, dims)[1]
    s = surface_sat(verts, tris, dims) if modes & SURFACE else np.zeros(dims, bool)
    f = solid_threshold(verts, tris, dims) if modes & SOLID else np.zeros(dims, bool)
    g = s | f
    return {"grid": g, "summary": (int(g.sum()), int(s.sum()), int(f.sum())) + counts}


def voxelize_slow(verts, tris, dims, modes):
    dims = tuple(int(d) for d in dims)
    counts = triangles(verts, tris, dims)[1]
    s = surface_clip(verts, tris, dims) if modes & SURFACE else np.zeros(dims, bool)
    f = solid_sign(verts, tris, dims) if modes & SOLID else np.zeros(dims, bool)
    g = s | f
    return {"grid": g, "summary": (int(g.sum()), int(s.sum()), int(f.sum())) + counts}


def pack(grid):
    """a bool [x, y, z] grid as region words (x in 32-bit words, rows y fastest, then z), padding bits 0"""
    d = grid.shape
    wpr = (d[0] + 31) // 32
    rows = np.zeros((d[2], d[1], wpr * 32), np.uint8)
    rows[:, :, :d[0]] = grid.transpose(2, 1, 0)
    return np.packbits(rows, axis=-1, bitorder="little").view("<u4").reshape(-1)


def unpack(words, dims):
    wpr = (dims[0] + 31) // 32
    b = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(dims[2], dims[1], wpr * 4), axis=-1, bitorder="little")
    return b[:, :, :dims[0]].transpose(2, 1, 0).astype(bool)


def workspace_bytes(dims, n_triangles):
    """the formula of include/vxrt.h"""
    if any(d < 1 or d > MAX_DIM for d in dims) or n_triangles > 1 << 24:
        return 0
    r = lambda n: (n + 255) // 256 * 256
    w = (dims[0] + 31) // 32 * dims[1] * dims[2]
    return r(4 * w) + r(4 * n_triangles) + r(8 * ((n_triangles + 255) // 256)) + 256


# ---- mesh generators: (int32 vertices (n, 3) in units of 1 / 256 voxel, uint32 triangles (m, 3)) ---------------------------------
def quantize(xyz):
    return np.rint(np.asarray(xyz, np.float64) * 256.0).astype(np.int32).reshape(-1, 3)


def _mesh(v, t):
    return np.ascontiguousarray(v, np.int32).reshape(-1, 3), np.ascontiguousarray(t, np.uint32).reshape(-1, 3)


def box_mesh(a, b):
    """the closed box with the corners a, b (units), 12 triangles, outward winding"""
    (x0, y0, z0), (x1, y1, z1) = a, b
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    t = [(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (0, 4, 7), (0, 7, 3), (1, 2, 6), (1, 6, 5)]
    return _mesh(v, t)


def octahedron(c, r):
    """centre c, radius r (units): 6 vertices on the axes, 8 triangles"""
    c = np.asarray(c, np.int64)
    v = [c + (r, 0, 0), c - (r, 0, 0), c + (0, r, 0), c - (0, r, 0), c + (0, 0, r), c - (0, 0, r)]
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return _mesh(v, t)


def icosphere(c, r, subdivisions):
    """centre c and radius r in voxels (floats); 20 * 4^subdivisions triangles, the shared vertices quantized once"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nt = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c3 in t:
            ab, bc, ca = m(a, b), m(b, c3), m(c3, a)
            nt += [(a, ab, ca), (b, bc, ab), (c3, ca, bc), (ab, bc, ca)]
        t = nt
    return _mesh(quantize(np.asarray(c, np.float64) + r * np.asarray(v)), t)


def torus(c, R, r, nu, nv):
    """centre c, radii R and r in voxels, the axis along y; 2 nu nv triangles"""
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    p = np.stack([(R + r * np.cos(w)) * np.cos(u), r * np.sin(w), (R + r * np.cos(w)) * np.sin(u)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + j % nv
    t = []
    for i in range(nu):
        for j in range(nv):
            t += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return _mesh(quantize(np.asarray(c, np.float64) + p), t)


def heightfield(nx, nz, cell, height, seed):
    """an open terrain patch over nx x nz cells of `cell` voxels, heights up to `height` voxels; 2 nx nz triangles"""
    rng = np.random.default_rng(seed)
    h = rng.random((nx + 1, nz + 1)) * height
    xs, zs = np.meshgrid(np.arange(nx + 1) * cell, np.arange(nz + 1) * cell, indexing="ij")
    p = np.stack([xs, h, zs], -1).reshape(-1, 3)
    idx = lambda i, j: i * (nz + 1) + j
    t = []
    for i in range(nx):
        for j in range(nz):
            t += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return _mesh(quantize(p), t)


def soup(n, dims, size, seed, margin=4):
    """n random triangles of about `size` voxels around centres within `margin` voxels of the region, some snapped to voxel
    boundaries and centres so that ties occur"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-margin, np.asarray(dims) + margin, (n, 1, 3))
    p = quantize((c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3)).reshape(n, 3, 3)
    snap = rng.random(n) < 0.3
    p[snap] = (p[snap] + 64) // 128 * 128
    return _mesh(p.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))
