"""numpy restatement of the nearest point on a mesh surface
(csrc/triangle_grid.hip: ucsa_triangle_cell_counts, ucsa_triangle_cell_pairs,
ucsa_nearest_triangle; ops.triangle_grid, ops.nearest_triangle).

``nearest_triangle`` is the definition: plain brute force over all faces, every
operation rounded to float32, no fused multiply-add.  It knows nothing of cells,
so the result cannot depend on the cell size, the grid's origin or the order of
the queries.

``nearest_triangle_grid`` is a model of the kernel's traversal: the same cell
arithmetic, the same registration of a face in the box of cells between its
corners' cells, the same rings, the same stop rule with the same margins, in the
same float32 expressions.  tests/test_surface_cpu.py holds it to the brute force
byte for byte, which proves the pruning before any GPU run.  Inside a ring the
kernel takes candidates one by one and the model takes them all at once; the
best candidate is the minimum of (dist2, face) over the visited set, which no
order and no repeated evaluation changes."""
import math

import numpy as np

from tests.nearest_numpy import (F, K, MAX_CELLS, NONE, ONE_PLUS_K, _f32, cell_coords,
                                 limit2_of)

# The slack of a wall distance is twice the point grid's (docs/DESIGN_NOTEBOOK.md,
# section NT): the closest point of a face is seven and a half roundings away
# from its corners, on top of the six of a point's wall distance.
KS = F(2.0) * K


def _faces(faces):
    return np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))


def valid_faces(V, Fc):
    """a face counts iff its three corner indices lie in [0, V) and the corners
    are finite"""
    nv = V.shape[0]
    ok = ((Fc >= 0) & (Fc < nv)).all(1)
    if nv:
        fin = np.isfinite(V).all(1)
        ok &= fin[np.clip(Fc, 0, nv - 1)].all(1)
    return ok


def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def closest(a, b, c):
    """The closest point of the triangle a, b, c (tuples of three float32 arrays,
    the query at the origin) -> (v, w, dist2): Ericson's regions, first match in
    the written order, every operation a float32 one."""
    sub = lambda x, y: (x[0] - y[0], x[1] - y[1], x[2] - y[2])
    neg = lambda x: (-x[0], -x[1], -x[2])
    with np.errstate(all="ignore"):
        ab, ac = sub(b, a), sub(c, a)
        d1, d2 = dot(ab, neg(a)), dot(ac, neg(a))
        d3, d4 = dot(ab, neg(b)), dot(ac, neg(b))
        d5, d6 = dot(ab, neg(c)), dot(ac, neg(c))
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        wb = e43 / (e43 + e56)
        den = one / ((va + vb) + vc)
        vi = vb * den
        wi = vc * den
        vi = np.where(vi < 0, zero, vi)
        vi = np.where(vi > 1, one, vi)
        t = one - vi
        wi = np.where(wi < 0, zero, wi)
        wi = np.where(wi > t, t, wi)
        v = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, one - wb], vi)
        w = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), wb], wi)
        p = [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]
        dist2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    assert dist2.dtype == F and v.dtype == F and w.dtype == F
    return v, w, dist2


def _bary(v, w):
    return np.stack([(F(1) - v) - w, v, w], -1).astype(F)


def nearest_triangle(verts, faces, queries, max_dist, chunk_pairs=1 << 20):
    """-> (face int32 [Q], dist2 float32 [Q], bary float32 [Q,3]); a face matches
    iff dist2 <= max_dist*max_dist (a NaN compares false); the smallest dist2
    wins, among equal ones the smallest face index; no match: -1, +inf and a
    zero bary row."""
    V, Fc, Q = _f32(verts), _faces(faces), _f32(queries)
    lim2 = limit2_of(max_dist)
    nq = Q.shape[0]
    face = np.full(nq, -1, np.int32)
    dist2 = np.full(nq, np.inf, F)
    bary = np.zeros((nq, 3), F)
    fid = np.nonzero(valid_faces(V, Fc))[0]
    if fid.size == 0 or nq == 0:
        return face, dist2, bary
    A, B, C = (V[Fc[fid, k]] for k in range(3))
    step = max(1, chunk_pairs // fid.size)
    for s in range(0, nq, step):
        q = Q[s:s + step]
        with np.errstate(all="ignore"):
            a, b, c = (tuple(X[None, :, k] - q[:, None, k] for k in range(3)) for X in (A, B, C))
            v, w, d2 = closest(a, b, c)
            ok = d2 <= lim2
        j = np.argmin(np.where(ok, d2, F(np.inf)), axis=1)        # the first minimum
        rows = np.arange(q.shape[0])
        hit = ok[rows, j]
        face[s:s + step] = np.where(hit, fid[j], -1)
        dist2[s:s + step] = np.where(hit, d2[rows, j], F(np.inf))
        bary[s:s + step] = np.where(hit[:, None], _bary(v[rows, j], w[rows, j]), F(0))
    return face, dist2, bary


# ---- the grid ---------------------------------------------------------------
def cell_cap(nf):
    return min(MAX_CELLS, max(4096, 64 * int(nf)))


def pair_cap(nf):
    return max(65536, 32 * int(nf))


def face_cell_boxes(V, Fc, ok, origin, cell, dims):
    """ucsa_triangle_cell_counts: per axis [pg_cell(min corner), pg_cell(max
    corner)] -> (c0 int64 [F,3], c1 int64 [F,3], counts int32 [F])"""
    nf = Fc.shape[0]
    if nf == 0 or V.shape[0] == 0:
        z = np.zeros((nf, 3), np.int64)
        return z, z.copy(), np.zeros(nf, np.int32)
    idx = np.clip(Fc, 0, V.shape[0] - 1)
    with np.errstate(all="ignore"):
        corners = V[idx]                                           # [F,3 corners,3]
        mn = np.minimum(np.minimum(corners[:, 0], corners[:, 1]), corners[:, 2])
        mx = np.maximum(np.maximum(corners[:, 0], corners[:, 1]), corners[:, 2])
    c0, _, _ = cell_coords(mn, origin, cell, dims)
    c1, _, _ = cell_coords(mx, origin, cell, dims)
    counts = np.where(ok, np.prod(c1 - c0 + 1, axis=1), 0)
    return c0, c1, counts.astype(np.int32)


def grid_shape(V, Fc, ok, lo, hi, cell=None):
    """origin, cell and dims (host arithmetic in float64 on float32 inputs; any
    choice gives the same search result).  The default cell is the lower median
    over the valid faces of the longest side of the face's box."""
    nf = Fc.shape[0]
    lo = np.asarray(lo, F).astype(np.float64)
    hi = np.asarray(hi, F).astype(np.float64)
    ext = hi - lo
    big = float(ext.max())
    if cell is None:
        if ok.any():
            corners = V[Fc[ok]]
            side = (corners.max(1) - corners.min(1)).max(1)        # float32
            cell = float(np.sort(side)[(side.size - 1) // 2])
        else:
            cell = big
    cell = float(F(max(float(cell), big / 1024.0, 1e-30)))   # a zero median: degenerate faces
    origin = lo.astype(F)
    while True:
        dims = tuple(int(math.floor(e / cell)) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= cell_cap(nf):
            counts = face_cell_boxes(V, Fc, ok, origin, F(cell), dims)[2]
            if int(counts.astype(np.int64).sum()) <= pair_cap(nf):
                return origin, F(cell), dims
        cell = float(F(cell * 1.25))


def triangle_grid(verts, faces, cell=None, origin=None):
    """ops.triangle_grid in numpy.  ``origin`` moves the grid's corner (at or
    below the vertices' box) to show that the result does not depend on it."""
    V, Fc = _f32(verts), _faces(faces)
    if cell is not None and not (float(cell) > 0 and math.isfinite(float(cell))):
        raise ValueError("cell must be positive and finite")
    ok = valid_faces(V, Fc)
    fin = np.isfinite(V).all(1)
    if fin.any():
        lo, hi = V[fin].min(0), V[fin].max(0)
    else:
        lo = hi = np.zeros(3, F)
    if origin is not None:
        lo = np.minimum(lo, np.asarray(origin, F))
    origin, cell, dims = grid_shape(V, Fc, ok, lo, hi, cell)
    c0, c1, counts = face_cell_boxes(V, Fc, ok, origin, cell, dims)
    cnt = counts.astype(np.int64)
    first = np.cumsum(cnt) - cnt                                   # exclusive scan
    P = int(cnt.sum())
    # ucsa_triangle_cell_pairs: face f writes its cells at first[f] ... in x, y, z order
    pf = np.repeat(np.arange(Fc.shape[0]), cnt)
    k = np.arange(P) - first[pf]
    ext = c1 - c0 + 1
    ny, nz = ext[pf, 1], ext[pf, 2]
    x = c0[pf, 0] + k // (ny * nz) if P else np.zeros(0, np.int64)
    y = c0[pf, 1] + (k // nz) % ny if P else np.zeros(0, np.int64)
    z = c0[pf, 2] + k % nz if P else np.zeros(0, np.int64)
    keys = ((x * dims[1] + y) * dims[2] + z).astype(np.int32)
    order = np.argsort(keys, kind="stable")
    ncells = dims[0] * dims[1] * dims[2]
    offsets = np.searchsorted(keys[order], np.arange(ncells + 1), side="left").astype(np.int32)
    sf = pf[order]
    rec = np.zeros((P, 12), np.int32)
    if P:
        for c in range(3):
            rec[:, 4 * c:4 * c + 3] = V[Fc[sf, c]].view(np.int32)
        rec[:, 3] = sf
    return {"origin": origin, "cell": cell, "dims": dims, "offsets": offsets,
            "records": rec.view(F), "n_pairs": P, "n_faces": int(Fc.shape[0]),
            "counts": counts, "first": first.astype(np.int32), "keys": keys,
            "pair_face": pf.astype(np.int32)}


def nearest_triangle_grid(verts, faces, queries, max_dist, cell=None, origin=None, stats=None):
    """The kernel's traversal.  Per query: rings r = 0, 1, ... of cells around
    the query's clamped cell, clipped to per-axis limits that start at the grid
    and close in as slabs of cells are proven too far; a ring's candidates
    compete by (dist2, face); the walk ends when no slab is left."""
    g = triangle_grid(verts, faces, cell, origin)
    Q = _f32(queries)
    lim2 = limit2_of(max_dist)
    nq, n = Q.shape[0], g["n_pairs"]
    o, h, dims = g["origin"], g["cell"], g["dims"]
    dm = np.asarray(dims, np.int64)
    rec, offsets = g["records"], g["offsets"].astype(np.int64)
    sidx = np.ascontiguousarray(rec[:, 3]).view(np.uint32) if n else np.zeros(0, np.uint32)
    best = np.full(nq, lim2, F)                  # B = min(best dist2, limit2)
    bidx = np.full(nq, NONE, np.uint32)
    visited = 0
    if nq and n:
        with np.errstate(all="ignore"):
            cq, finite, _ = cell_coords(Q, o, h, dims)
            top = o + dm.astype(F) * h                                # the box's far corner
            S = KS * ((np.abs(o) + np.abs(top))[None, :] + np.abs(Q))  # slack per query and axis
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
                    a, b, c = (tuple(rec[k, 4 * s + t] - Q[qi, t] for t in range(3))
                               for s in range(3))
                    _, _, d2 = closest(a, b, c)
                    j = sidx[k]
                    take = (d2 < best[qi]) | ((d2 == best[qi]) & (j < bidx[qi]))
                qi, d2, j = qi[take], d2[take], j[take]
                low = np.full(nq, np.inf, F)                      # each query's least dist2 first:
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
                for ax in range(3):
                    m_hi = cq[A, ax] + r + 1                         # first cell of the far slab
                    has = m_hi <= hi[A, ax]
                    gap = ((o[ax] + m_hi.astype(F) * h) - Q[A, ax]) - S[A, ax]
                    cut = has & (gap > 0) & (gap * gap > bk)
                    hi[A, ax] = np.where(cut, cq[A, ax] + r, hi[A, ax])
                    left |= has & ~cut
                    m_lo = cq[A, ax] - r - 1                         # last cell of the near slab
                    has = m_lo >= lo[A, ax]
                    gap = (Q[A, ax] - (o[ax] + (m_lo + 1).astype(F) * h)) - S[A, ax]
                    cut = has & (gap > 0) & (gap * gap > bk)
                    lo[A, ax] = np.where(cut, cq[A, ax] - r, lo[A, ax])
                    left |= has & ~cut
            active[A[~left]] = False
            r += 1
    if stats is not None:
        stats["cells_visited"] = visited
        stats["cells"] = int(np.prod(dims))
    hit = bidx != NONE
    face = np.where(hit, bidx, 0).astype(np.int64).astype(np.int32)
    face[~hit] = -1
    dist2 = np.where(hit, best, F(np.inf)).astype(F)
    bary = np.zeros((nq, 3), F)
    if hit.any():
        # the winner's weights: the same expressions on the same operands as in the walk
        V, Fc = _f32(verts), _faces(faces)
        qh = Q[hit]
        with np.errstate(all="ignore"):
            a, b, c = (tuple(V[Fc[face[hit], s], t] - qh[:, t] for t in range(3)) for s in range(3))
            v, w, d2 = closest(a, b, c)
        assert d2.tobytes() == dist2[hit].tobytes()
        bary[hit] = _bary(v, w)
    return face, dist2, bary
