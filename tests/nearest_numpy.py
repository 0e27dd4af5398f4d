"""numpy restatement of the nearest-point search (csrc/point_grid.hip:
ucsa_point_cell_keys, ucsa_nearest_point; ops.point_grid, ops.nearest_point).

``nearest_point`` is the definition: plain brute force, every operation rounded
to float32, no fused multiply-add.  It knows nothing of cells, so the result
cannot depend on the cell size, the grid's origin or the order of the queries.

``nearest_point_grid`` is a model of the kernel's traversal: the same cell
arithmetic, the same rings, the same stop rule with the same margins, in the
same float32 expressions.  The traversal itself is ``ring_walk``, which
tests/surface_numpy.py calls too, as both kernels call pg_walk.  tests/test_nearest_cpu.py holds it to the brute
force byte for byte, which proves the pruning before any GPU run.  Inside a
ring the kernel takes candidates one by one and the model takes them all at
once; the best candidate is the minimum of (d2, index) over the visited set,
which no order changes."""
import math

import numpy as np

F = np.float32
MAX_CELLS = 1 << 24
NONE = np.uint32(0xFFFFFFFF)
# The margins of the stop rule (docs/DESIGN_NOTEBOOK.md, section NN).  K = 16
# units in the last place: a wall's position, the gap to it and d2 are each off
# by a few ulp of the coordinates involved, never by 16.
K = F(2.0 ** -20)
ONE_PLUS_K = F(1.0) + K


def _f32(a, cols=3):
    return np.ascontiguousarray(np.asarray(a, F).reshape(-1, cols))


def limit2_of(max_dist):
    md = F(max_dist)
    with np.errstate(over="ignore"):
        lim2 = md * md
    if not (np.isfinite(md) and md > 0 and np.isfinite(lim2)):
        raise ValueError("max_dist must be positive, finite, and its square finite in float32")
    return lim2


def nearest_point(points, queries, max_dist, chunk_pairs=1 << 22):
    """-> (index int32 [Q], dist2 float32 [Q]).  d2 = (dx*dx + dy*dy) + dz*dz with
    dx = q.x - p.x ..., all float32; j matches i iff d2 <= max_dist*max_dist (a
    NaN compares false); the smallest d2 wins, among equal d2 the smallest j;
    no match: -1 and +inf."""
    P, Q = _f32(points), _f32(queries)
    lim2 = limit2_of(max_dist)
    n, nq = P.shape[0], Q.shape[0]
    index = np.full(nq, -1, np.int32)
    dist2 = np.full(nq, np.inf, F)
    if n == 0 or nq == 0:
        return index, dist2
    step = max(1, chunk_pairs // n)
    for a in range(0, nq, step):
        q = Q[a:a + step]
        with np.errstate(all="ignore"):
            dx = q[:, None, 0] - P[None, :, 0]
            dy = q[:, None, 1] - P[None, :, 1]
            dz = q[:, None, 2] - P[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = d2 <= lim2
        assert d2.dtype == F
        j = np.argmin(np.where(ok, d2, F(np.inf)), axis=1)      # the first minimum
        rows = np.arange(q.shape[0])
        hit = ok[rows, j]                                       # lim2 is finite: a match is < inf
        index[a:a + step] = np.where(hit, j, -1)
        dist2[a:a + step] = np.where(hit, d2[rows, j], F(np.inf))
    return index, dist2


# ---- the grid ---------------------------------------------------------------
def cell_cap(n):
    """the most cells a grid of n points gets: more cells than 64 per point buy
    nothing and cost an offset each"""
    return min(MAX_CELLS, max(4096, 64 * int(n)))


def grid_shape(lo, hi, n, cell=None):
    """origin, cell and dims from the finite points' box (host arithmetic in
    float64 on float32 inputs; any choice gives the same search result)."""
    lo = np.asarray(lo, F).astype(np.float64)
    hi = np.asarray(hi, F).astype(np.float64)
    ext = hi - lo
    big = float(ext.max())
    if cell is None:
        pad = ext + max(big, 1e-30) * 1e-3
        cell = (float(np.prod(pad)) / max(int(n), 1)) ** (1.0 / 3.0)
    cell = float(cell)
    if not (cell > 0 and math.isfinite(cell)):
        raise ValueError("cell must be positive and finite")
    cell = float(F(max(cell, big / 1024.0, 1e-30)))
    cap = cell_cap(n)
    while True:
        dims = [int(math.floor(e / cell)) + 1 for e in ext]
        if dims[0] * dims[1] * dims[2] <= cap:
            return lo.astype(F), F(cell), tuple(dims)
        cell = float(F(cell * 1.25))


def cell_coords(x, origin, cell, dims):
    """float32 [M,3] -> (int64 [M,3] clamped cell coordinates, finite [M], inside
    [M]); t = (x - origin) / cell in float32, clamped as a float, then floored."""
    with np.errstate(all="ignore"):
        t = (x - origin[None, :]) / cell
        finite = np.isfinite(x).all(1)
        top = np.asarray(dims, F)[None, :] - F(1)
        inside = finite & ((t >= 0) & (t < np.asarray(dims, F)[None, :])).all(1)
        tc = np.minimum(np.maximum(np.where(np.isnan(t), F(0), t), F(0)), top)
    return np.floor(tc).astype(np.int64), finite, inside


def cell_keys(x, origin, cell, dims, clamp=True):
    """ucsa_point_cell_keys: int32 [M]"""
    c, finite, inside = cell_coords(_f32(x), origin, cell, dims)
    ncells = dims[0] * dims[1] * dims[2]
    key = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    return np.where(finite if clamp else inside, key, ncells).astype(np.int32)


def point_grid(points, cell=None, origin=None):
    """ops.point_grid in numpy.  ``origin`` moves the grid's corner (at or below
    the points' box) to show that the result does not depend on it."""
    P = _f32(points)
    ok = np.isfinite(P).all(1)
    n = P.shape[0]
    if ok.any():
        lo, hi = P[ok].min(0), P[ok].max(0)
    else:
        lo = hi = np.zeros(3, F)
    if origin is not None:
        lo = np.minimum(lo, np.asarray(origin, F))
    origin, cell, dims = grid_shape(lo, hi, n, cell)
    keys = cell_keys(P, origin, cell, dims)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    ncells = dims[0] * dims[1] * dims[2]
    offsets = np.searchsorted(keys[order], np.arange(ncells + 1), side="left").astype(np.int32)
    sp = np.empty((n, 4), np.int32)
    sp[:, :3] = P[order].view(np.int32)
    sp[:, 3] = order
    return {"origin": origin, "cell": cell, "dims": dims, "offsets": offsets, "order": order,
            "sorted_points": sp.view(F), "n": n}


def ring_walk(origin, cell, dims, offsets, n, Q, lim2, ks, candidate):
    """The kernels' traversal (pg_walk in csrc/cell_grid.h), once for both
    searches -> (best float32 [Q], bidx uint32 [Q], cells visited).  Per query:
    rings r = 0, 1, ... of cells around the query's clamped cell, clipped to
    per-axis limits that start at the grid and close in as slabs of cells are
    proven too far; a ring's candidates compete by (d2, index); the walk ends
    when no slab is left.  ``n`` is the number of sorted candidates, ``ks`` the
    slack of a wall distance (K for points, KS for faces) and ``candidate(qi, k)``
    -> (d2 float32, j uint32) scores the candidates at sorted positions ``k``
    for the queries ``qi``."""
    o, h = origin, cell
    nq = Q.shape[0]
    dm = np.asarray(dims, np.int64)
    offsets = offsets.astype(np.int64)
    best = np.full(nq, lim2, F)                  # B = min(best d2, limit2)
    bidx = np.full(nq, NONE, np.uint32)
    visited = 0
    if nq and n:
        with np.errstate(all="ignore"):
            cq, finite, _ = cell_coords(Q, o, h, dims)
            top = o + dm.astype(F) * h                               # the box's far corner
            S = ks * ((np.abs(o) + np.abs(top))[None, :] + np.abs(Q))  # slack per query and axis
            e = np.maximum(np.maximum(o[None, :] - Q, Q - top[None, :]) - S, F(0))
            out2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            far = out2 > lim2 * ONE_PLUS_K
        active = finite & ~far
        lo = np.zeros((nq, 3), np.int64)
        hi = np.broadcast_to(dm - 1, (nq, 3)).copy()
        r = 0
        while active.any():
            A = np.nonzero(active)[0]
            d = np.arange(-r, r + 1)
            DX, DY = [a.reshape(-1) for a in np.meshgrid(d, d, indexing="ij")]
            edge = (np.abs(DX) == r) | (np.abs(DY) == r)
            x = cq[A, 0, None] + DX[None, :]
            y = cq[A, 1, None] + DY[None, :]
            inxy = ((x >= lo[A, 0, None]) & (x <= hi[A, 0, None]) &
                    (y >= lo[A, 1, None]) & (y <= hi[A, 1, None]))
            zc, zl, zh = cq[A, 2, None], lo[A, 2, None], hi[A, 2, None]
            runs = []                                               # (mask, z0, z1) per column
            runs.append((inxy & edge[None, :], np.maximum(zc - r, zl) + 0 * x,
                         np.minimum(zc + r, zh) + 0 * x))
            if r > 0:
                runs.append((inxy & ~edge[None, :] & (zc - r >= zl), zc - r + 0 * x, zc - r + 0 * x))
                runs.append((inxy & ~edge[None, :] & (zc + r <= zh), zc + r + 0 * x, zc + r + 0 * x))
            qs, bs, es = [], [], []
            for m, z0, z1 in runs:
                m = m & (z0 <= z1)
                row = (x[m] * dims[1] + y[m]) * dims[2]
                qs.append(np.broadcast_to(A[:, None], m.shape)[m])
                bs.append(np.clip(offsets[row + z0[m]], 0, n))
                es.append(np.clip(offsets[row + z1[m] + 1], 0, n))
                visited += int((z1[m] - z0[m] + 1).sum())
            qs, bs, es = np.concatenate(qs), np.concatenate(bs), np.concatenate(es)
            cnt = np.maximum(es - bs, 0)
            if cnt.sum():
                qi = np.repeat(qs, cnt)
                k = np.repeat(bs - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
                with np.errstate(all="ignore"):
                    d2, j = candidate(qi, k)
                    take = (d2 < best[qi]) | ((d2 == best[qi]) & (j < bidx[qi]))
                qi, d2, j = qi[take], d2[take], j[take]
                low = np.full(nq, np.inf, F)                      # each query's least d2 first:
                np.minimum.at(low, qi, d2)                        # few candidates reach the sort
                take = d2 == low[qi]
                qi, d2, j = qi[take], d2[take], j[take]
                first = np.lexsort((j, d2, qi))
                qi, d2, j = qi[first], d2[first], j[first]
                head = np.ones(qi.size, bool)
                head[1:] = qi[1:] != qi[:-1]
                best[qi[head]] = d2[head]
                bidx[qi[head]] = j[head]
            # the stop rule: a slab of unvisited cells beyond a wall is dropped once
            # the wall is provably farther than B, strictly and with the margins
            left = np.zeros(A.size, bool)
            with np.errstate(all="ignore"):
                bk = best[A] * ONE_PLUS_K
                for a in range(3):
                    m_hi = cq[A, a] + r + 1                          # first cell of the far slab
                    has = m_hi <= hi[A, a]
                    gap = ((o[a] + m_hi.astype(F) * h) - Q[A, a]) - S[A, a]
                    cut = has & (gap > 0) & (gap * gap > bk)
                    hi[A, a] = np.where(cut, cq[A, a] + r, hi[A, a])
                    left |= has & ~cut
                    m_lo = cq[A, a] - r - 1                          # last cell of the near slab
                    has = m_lo >= lo[A, a]
                    gap = (Q[A, a] - (o[a] + (m_lo + 1).astype(F) * h)) - S[A, a]
                    cut = has & (gap > 0) & (gap * gap > bk)
                    lo[A, a] = np.where(cut, cq[A, a] - r, lo[A, a])
                    left |= has & ~cut
            active[A[~left]] = False
            r += 1
    return best, bidx, visited


def _search_result(best, bidx, dims, visited, stats):
    """(index int32, dist2 float32) of a walk's (best, bidx), and the stats"""
    if stats is not None:
        stats["cells_visited"] = visited
        stats["cells"] = int(np.prod(dims))
    hit = bidx != NONE
    index = np.where(hit, bidx, 0).astype(np.int64).astype(np.int32)
    index[~hit] = -1
    return index, np.where(hit, best, F(np.inf)).astype(F)


def nearest_point_grid(points, queries, max_dist, cell=None, origin=None, stats=None):
    """ucsa_nearest_point's traversal: ``ring_walk`` over ``point_grid``'s sorted
    points with the point search's candidate test and slack K."""
    g = point_grid(points, cell, origin)
    Q = _f32(queries)
    sp = g["sorted_points"]
    sidx = sp[:, 3].view(np.uint32)

    def candidate(qi, k):
        dx = Q[qi, 0] - sp[k, 0]
        dy = Q[qi, 1] - sp[k, 1]
        dz = Q[qi, 2] - sp[k, 2]
        return (dx * dx + dy * dy) + dz * dz, sidx[k]

    best, bidx, visited = ring_walk(g["origin"], g["cell"], g["dims"], g["offsets"], g["n"], Q,
                                    limit2_of(max_dist), K, candidate)
    return _search_result(best, bidx, g["dims"], visited, stats)
