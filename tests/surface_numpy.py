"""numpy restatement of the nearest point on a mesh surface
(csrc/triangle_grid.hip: ucsa_triangle_cell_counts, ucsa_triangle_cell_pairs,
ucsa_nearest_triangle; ops.triangle_grid, ops.nearest_triangle).

``nearest_triangle`` is the definition: plain brute force over all faces, every
operation rounded to float32, no fused multiply-add.  It knows nothing of cells,
so the result cannot depend on the cell size, the grid's origin or the order of
the queries.

``nearest_triangle_grid`` is a model of the kernel's traversal: the same cell
arithmetic, the same registration of a face in the box of cells between its
corners' cells, and the rings and the stop rule of tests/nearest_numpy.py's
``ring_walk`` with this search's candidate test and margin, in the same float32
expressions.  tests/test_surface_cpu.py holds it to the brute force
byte for byte, which proves the pruning before any GPU run.  Inside a ring the
kernel takes candidates one by one and the model takes them all at once; the
best candidate is the minimum of (dist2, face) over the visited set, which no
order and no repeated evaluation changes."""
import math

import numpy as np

from tests.nearest_numpy import (F, K, MAX_CELLS, _f32, _search_result, cell_coords, limit2_of,
                                 ring_walk)

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
    """ucsa_nearest_triangle's traversal: ``ring_walk`` over ``triangle_grid``'s
    records with the face search's candidate test and slack KS."""
    g = triangle_grid(verts, faces, cell, origin)
    Q = _f32(queries)
    rec = g["records"]
    sidx = np.ascontiguousarray(rec[:, 3]).view(np.uint32)

    def candidate(qi, k):
        a, b, c = (tuple(rec[k, 4 * s + t] - Q[qi, t] for t in range(3)) for s in range(3))
        return closest(a, b, c)[2], sidx[k]

    best, bidx, visited = ring_walk(g["origin"], g["cell"], g["dims"], g["offsets"],
                                    g["n_pairs"], Q, limit2_of(max_dist), KS, candidate)
    face, dist2 = _search_result(best, bidx, g["dims"], visited, stats)
    hit = face >= 0
    nq = Q.shape[0]
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
