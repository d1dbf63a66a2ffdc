"""Two restatements of the navigation-field contract (include/vxrt.h, vxrt_nav_field) on a bool [x, y, z] world grid:
  nav_field        pure numpy: dense free / supported / walkable booleans, a level-by-level reverse BFS with one shifted
                   frontier and one sweep mask per move, next from dist;
  nav_field_scipy  an explicit edge list (one numpy pass per move type over every cell), the reversed graph searched from
                   the goal nodes with scipy.sparse.csgraph.shortest_path(unweighted=True) from one extra source joined to
                   every goal node (the minimum over the goals), next as the first edge in code order one level down.
Both return {"walkable": bool [x, y, z], "dist": uint32 [x, y, z] (0xFFFFFFFF unreachable), "next": uint8 [x, y, z],
"summary": (nodes, goals_used, goals_ignored, reached, max_dist_found, levels)}.  decode_paths follows next codes as
vxrt_nav_paths does.  TEST INFRASTRUCTURE ONLY: imported by tests/ alone."""
from __future__ import annotations

import numpy as np

from oracle import ref_region

UNREACHED = 0xFFFFFFFF
NONE = 0xFF
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))  # (dx, dz): +x, -x, +z, -z
AT_GOAL, NO_PATH, TRUNCATED, OUTSIDE = 0, 1, 2, 3


def moves(agent):
    """[(code, dx, dy, dz)] in code order"""
    w, h, climb, drop = agent
    dys = [0] + list(range(1, climb + 1)) + [-j for j in range(1, drop + 1)]
    per = 1 + climb + drop
    return [(1 + k * per + i, dx, dy, dz) for k, (dx, dz) in enumerate(DIRS) for i, dy in enumerate(dys)]


def free_supported(world, origin, dims, agent):
    """free and supported over B, read from the halo box of the world"""
    w, h = agent[0], agent[1]
    X, Y, Z = dims
    halo = ref_region.read_region(world, (origin[0], origin[1] - 1, origin[2]), (X + w - 1, Y + h, Z + w - 1))
    empty = ~halo
    ex = np.ones((X, Y + h, Z + w - 1), bool)
    dx = np.zeros((X, Y + h, Z + w - 1), bool)
    for i in range(w):
        ex &= empty[i:i + X]
        dx |= halo[i:i + X]
    fy = np.ones((X, Y, Z + w - 1), bool)
    for j in range(h):
        fy &= ex[:, 1 + j:1 + j + Y]
    free = np.ones((X, Y, Z), bool)
    sup = np.zeros((X, Y, Z), bool)
    for k in range(w):
        free &= fy[:, :, k:k + Z]
        sup |= dx[:, :Y, k:k + Z]
    return free, sup


def _shift(a, off):
    """b[c] = a[c + off], False outside"""
    b = np.zeros_like(a)
    src, dst = [], []
    for k, o in enumerate(off):
        n = a.shape[k]
        if abs(o) >= n:
            return b
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n - max(o, 0)))
    b[tuple(dst)] = a[tuple(src)]
    return b


def _goal_nodes(walk, origin, goals):
    g = np.zeros(walk.shape, bool)
    used = ignored = 0
    for c in np.asarray(goals, np.int64).reshape(-1, 3):
        p = c - np.asarray(origin, np.int64)
        if (p >= 0).all() and (p < walk.shape).all() and walk[tuple(p)]:
            g[tuple(p)] = True
            used += 1
        else:
            ignored += 1
    return g, used, ignored


def _sweeps(free, agent):
    """A[k][c] = free(c + (0, i, 0)) for i = 1 .. k (k = 0: all True)"""
    K = max(agent[2], agent[3])
    A = [np.ones(free.shape, bool)]
    for k in range(1, K + 1):
        A.append(A[-1] & _shift(free, (0, k, 0)))
    return A


def _summary(walk, dist, used, ignored):
    r = dist != UNREACHED
    mx = int(dist[r].max()) if r.any() else 0
    return (int(walk.sum()), used, ignored, int(r.sum()), mx, mx + 1 if used else 0)


def nav_field(world, origin, dims, agent, goals, max_dist=1 << 24) -> dict:
    free, sup = free_supported(world, origin, dims, agent)
    walk = free & sup
    A = _sweeps(free, agent)
    g, used, ignored = _goal_nodes(walk, origin, goals)
    dist = np.full(walk.shape, UNREACHED, np.uint32)
    dist[g] = 0
    vis, front, lv = g.copy(), g.copy(), 0
    while front.any() and lv < max_dist:
        pred = np.zeros_like(walk)
        for _, dx, dy, dz in moves(agent):
            if dy >= 0:   # c -> t = c + (dx, dy, dz), free above c
                pred |= A[dy] & _shift(front, (dx, dy, dz))
            else:         # free above t up to c's row
                pred |= _shift(front & A[-dy], (dx, dy, dz))
        new = pred & walk & ~vis
        lv += 1
        dist[new] = lv
        vis |= new
        front = new
    nxt = np.full(walk.shape, NONE, np.uint8)
    nxt[dist == 0] = 0
    D = dist.astype(np.int64)
    todo = (dist != UNREACHED) & (dist != 0)
    for code, dx, dy, dz in moves(agent):
        Dt = _shift(np.where(dist == UNREACHED, -5, D), (dx, dy, dz))
        inb = _shift(np.ones_like(walk), (dx, dy, dz))
        ok = inb & (Dt == D - 1) & (A[dy] if dy >= 0 else _shift(A[-dy], (dx, dy, dz)))
        hit = todo & ok
        nxt[hit] = code
        todo &= ~hit
    return {"walkable": walk, "dist": dist, "next": nxt, "summary": _summary(walk, dist, used, ignored)}


def have_scipy() -> bool:
    try:
        import scipy.sparse.csgraph  # noqa: F401
        return True
    except ImportError:
        return False


def edges(walk, free, agent):
    """the valid moves as (source cell, target cell, code) arrays of flat region indices, sorted by source then code"""
    X, Y, Z = walk.shape
    x, y, z = np.nonzero(walk)
    src, dst, cod = [], [], []
    fidx = lambda a, b, c: a + X * (b + Y * c)
    for code, dx, dy, dz in moves(agent):
        tx, ty, tz = x + dx, y + dy, z + dz
        ok = (tx >= 0) & (tx < X) & (ty >= 0) & (ty < Y) & (tz >= 0) & (tz < Z)
        ok[ok] &= walk[tx[ok], ty[ok], tz[ok]]
        for k in range(1, dy + 1):               # rising: free above the start
            ok[ok] &= free[x[ok], y[ok] + k, z[ok]]
        for k in range(dy + 1, 1):               # falling: free beside the start, down to the target
            ok[ok] &= free[tx[ok], y[ok] + k, tz[ok]]
        src.append(fidx(x[ok], y[ok], z[ok]))
        dst.append(fidx(tx[ok], ty[ok], tz[ok]))
        cod.append(np.full(int(ok.sum()), code))
    src, dst, cod = np.concatenate(src), np.concatenate(dst), np.concatenate(cod)
    o = np.lexsort((cod, src))
    return src[o], dst[o], cod[o]


def nav_field_scipy(world, origin, dims, agent, goals, max_dist=1 << 24) -> dict:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    free, sup = free_supported(world, origin, dims, agent)
    walk = free & sup
    X, Y, Z = walk.shape
    n = X * Y * Z
    src, dst, cod = edges(walk, free, agent)
    g, used, ignored = _goal_nodes(walk, origin, goals)
    flat = lambda a: a.transpose(2, 1, 0).reshape(-1)
    grid = lambda a: a.reshape(Z, Y, X).transpose(2, 1, 0)
    gi = np.nonzero(flat(g))[0]
    dist = np.full(n, UNREACHED, np.uint32)
    if len(gi):
        rs = np.concatenate([dst, np.full(len(gi), n)])  # node n: the source, one edge to every goal node
        rd = np.concatenate([src, gi])
        rev = csr_matrix((np.ones(len(rs)), (rs, rd)), shape=(n + 1, n + 1))
        d = shortest_path(rev, unweighted=True, indices=n)[:n] - 1
        fin = np.isfinite(d) & (d <= max_dist)
        dist[fin] = d[fin].astype(np.uint32)
    nxt = np.full(n, NONE, np.uint8)
    nxt[dist == 0] = 0
    Ds, Dt = dist[src].astype(np.int64), dist[dst].astype(np.int64)
    good = (dist[src] != UNREACHED) & (Ds > 0) & (dist[dst] != UNREACHED) & (Dt == Ds - 1)
    s, c = src[good], cod[good]
    first = np.ones(len(s), bool)
    first[1:] = s[1:] != s[:-1]
    nxt[s[first]] = c[first]
    dist, nxt = grid(dist), grid(nxt)
    return {"walkable": walk, "dist": dist, "next": nxt, "summary": _summary(walk, dist, used, ignored)}


def decode_paths(nxt, origin, agent, starts, max_steps):
    """vxrt_nav_paths on the host: (cells (n, max_steps + 1, 3), lengths, status)"""
    dims = nxt.shape
    mv = {code: (dx, dy, dz) for code, dx, dy, dz in moves(agent)}
    starts = np.asarray(starts, np.int64).reshape(-1, 3)
    cells = np.zeros((len(starts), max_steps + 1, 3), np.int32)
    lengths = np.zeros(len(starts), np.int32)
    status = np.zeros(len(starts), np.int32)
    o = np.asarray(origin, np.int64)
    for i, s in enumerate(starts):
        p = s.copy()
        inside = lambda q: bool(((q - o) >= 0).all() and ((q - o) < dims).all())
        path = [p.copy()]
        if not inside(p):
            st = OUTSIDE
        else:
            while True:
                code = int(nxt[tuple(p - o)])
                if code == 0:
                    st = AT_GOAL
                    break
                if code not in mv:
                    st = NO_PATH
                    break
                if len(path) - 1 == max_steps:
                    st = TRUNCATED
                    break
                q = p + mv[code]
                if not inside(q):
                    st = NO_PATH
                    break
                p = q
                path.append(p.copy())
        lengths[i] = len(path) - 1  # every move changes x or z
        path += [path[-1]] * (max_steps + 1 - len(path))
        cells[i] = np.asarray(path, np.int32)
        status[i] = st
    return cells, lengths, status


def snake_world(X, Z, wall=4):
    """a floor at y = 0 and walls `wall` voxels high that leave a one-cell serpentine corridor: rows z = 0, 2, 4, .. open,
    rows z = 1, 3, .. walled but for one gap at alternating ends -- a path of about X * Z / 2 moves for a small agent"""
    v = np.zeros((X, wall + 4, Z), bool)
    v[:, 0, :] = True
    for k, z in enumerate(range(1, Z, 2)):
        v[:, 1:1 + wall, z] = True
        v[X - 1 if k % 2 == 0 else 0, 1:1 + wall, z] = False
    return v
